"""hpc.sampler — fused sampler at the end of a decode step (reference hpc/sampler.py:8-330)."""
from enum import IntEnum
from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from . import _C  # noqa: F401  (loads the libraries that register torch.ops.hpc.*)


class SoftmaxPolicy(IntEnum):
    """Where the sampler runs softmax (at most once per step; reference hpc/sampler.py:8-28):
    NONE — top-k / Gumbel-max work on logits; BEFORE_TOPK — softmax over the full vocabulary, top-k and
    top-p on probabilities; AFTER_TOPK — top-k on logits, softmax over the surviving top-k, top-p on it.
    top-p requires a policy != NONE."""

    NONE = 0
    BEFORE_TOPK = 1
    AFTER_TOPK = 2


def _to_tensor_scalar_tuple(x) -> Tuple[Optional[Tensor], Union[int, float]]:
    if isinstance(x, torch.Tensor):
        if x.dtype == torch.float:
            return (x, 0.0)
        if x.dtype in (torch.int32, torch.int64):
            return (x, 0)
        raise ValueError(f"Unsupported dtype {x.dtype}")
    return (None, x)


def fused_sampler(
    logits: Tensor,
    *,
    penalty_mask: Optional[Tensor] = None,
    slot_id: Optional[Tensor] = None,
    repetition_penalty: Union[Tensor, float] = 0.0,
    temperature: Union[Tensor, float] = 0.0,
    softmax_policy: SoftmaxPolicy = SoftmaxPolicy.NONE,
    topk: Union[Tensor, int] = 0,
    topp: Union[Tensor, float] = 0.0,
    max_topk: int = 32,
    gumbel_noise: Optional[Tensor] = None,
    draft_token_ids: Optional[Tensor] = None,
    seed: int = 0,
) -> Tensor:
    """repetition_penalty -> temperature -> [softmax] -> topk -> [softmax] -> topp -> Gumbel-max ->
    penalty write-back; every stage except the final Gumbel-max is optional and sampling always happens
    inside the top-``max_topk`` (32 / 64) candidates.

    logits [B, V] float32 / bfloat16 (inner stride 1; V % 8 == 0); penalty_mask [MAX_BS, ceil(V/8)] uint8
    bit mask + slot_id [B] int32 (together or not at all; the sampled token's bit is OR-ed in);
    repetition_penalty / temperature / topp: scalar or [B] float32 (0 disables); topk: scalar or [B]
    int32/int64 (<= max_topk; 0 = max_topk); gumbel_noise [B, V] float32 makes sampling reproducible
    against the PyTorch model, otherwise Philox noise is drawn from ``seed`` (> 0); draft_token_ids [B]
    int64 (-1 = none) masks one token per row, temperature-only fast path only.
    Returns token_ids int32 [B, 1].  (reference hpc/sampler.py:42-200)"""
    if isinstance(softmax_policy, int) and not isinstance(softmax_policy, SoftmaxPolicy):
        softmax_policy = SoftmaxPolicy(softmax_policy)
    if max_topk not in (32, 64):
        raise ValueError(f"fused_sampler: max_topk must be 32 or 64, got {max_topk}.")

    def _is_scalar_zero(x):
        return (not isinstance(x, Tensor)) and float(x) == 0.0

    temp_is_tensor = isinstance(temperature, Tensor)
    fast_path = (
        penalty_mask is None
        and slot_id is None
        and _is_scalar_zero(repetition_penalty)
        and _is_scalar_zero(topp)
        and (not isinstance(topk, Tensor))
        and int(topk) == 0
        and softmax_policy == SoftmaxPolicy.NONE
        and (temp_is_tensor or float(temperature) > 0.0)
    )
    if fast_path:
        temp_tensor, temp_scalar = _to_tensor_scalar_tuple(temperature)
        return torch.ops.hpc.fused_sampler_temperature_sample(
            logits, temp_tensor, float(temp_scalar), gumbel_noise, draft_token_ids, seed)
    if draft_token_ids is not None:
        raise ValueError(
            "draft_token_ids currently requires the temperature-only fast path. Disable the other sampler features "
            "(penalty_mask/slot_id/repetition_penalty/topk/topp/softmax_policy) to use draft-mask sampling.")
    return torch.ops.hpc.fused_sampler(
        logits, penalty_mask, slot_id,
        *_to_tensor_scalar_tuple(repetition_penalty),
        *_to_tensor_scalar_tuple(temperature),
        int(softmax_policy),
        *_to_tensor_scalar_tuple(topk),
        *_to_tensor_scalar_tuple(topp),
        max_topk, gumbel_noise, seed,
    )


@torch.library.register_fake("hpc::fused_sampler")
def _fused_sampler_fake(logits, penalty_mask, slot_id, repetition_penalty, repetition_penalty_val, temperature,
                        temperature_val, softmax_policy, topk, topk_val, topp, topp_val, max_topk,
                        gumbel_noise=None, seed=0):
    return torch.empty((logits.shape[0], 1), dtype=torch.int32, device=logits.device)


@torch.library.register_fake("hpc::fused_sampler_temperature_sample")
def _fused_sampler_temperature_fake(logits, temperature, temperature_val, gumbel_noise=None, draft_token_ids=None,
                                    seed=0):
    return torch.empty((logits.shape[0], 1), dtype=torch.int32, device=logits.device)


def speculative_verify(
    logits: Tensor,
    draft_token_ids: Tensor,
    *,
    temperature: Union[Tensor, float] = 1.0,
    uniform_samples: Optional[Tensor] = None,
    gumbel_noise: Optional[Tensor] = None,
    seed: int = 0,
    output_token_ids: Optional[Tensor] = None,
    num_accepted: Optional[Tensor] = None,
) -> Tuple[Tensor, Tensor]:
    """Draft-token verification at the end of a speculative (MTP) decode step, in one pass over the logits: how many
    of a request's K drafts are accepted, the recovered token at the first rejection, or the bonus token when all are
    accepted.  No reference counterpart (torch.ops.hpc_spec.speculative_verify); semantics = PyTorch
    (tests/spec_verify_ref.py).

    logits [B * (K + 1), V] float32 / bfloat16 (inner stride 1, row stride >= V, V % 8 == 0, V < 2^20, never written):
    row b * (K + 1) + j is the target model's distribution for position j of request b.  draft_token_ids int64 [B, K],
    0 <= K <= 15: the first entry < 0 or >= V ends the request's drafts, n_b = number of leading valid entries; logits rows
    past n_b are not read.  temperature: scalar or float32 [B], one per request; 0 = greedy for that request (negative or
    NaN: unspecified).  Per request, with T its temperature, for j = 0 .. n_b - 1, r = b * (K + 1) + j, d = draft[b, j]:
        T > 0:  accept iff uniform_samples[b, j] < softmax(logits[r].float() / T)[d]
        T == 0: accept iff d == argmax(logits[r]), ties -> smaller token id
    First rejection at j: out[b, j] = argmax(logits[r].float() / T + gumbel_noise[r]) with entry d at -inf, ties -> smaller
    id - exactly what fused_sampler(row, temperature=T, gumbel_noise=..., draft_token_ids=d) returns - or argmax(logits[r])
    when T == 0; out[b, :j] are the accepted drafts, out[b, j+1:] = -1, num_accepted[b] = j.  All accepted:
    out[b, n_b] is sampled from row b * (K + 1) + n_b without a mask (arg-max when T == 0), num_accepted[b] = n_b, later
    entries are -1.

    This is rejection sampling against a draft distribution that puts probability 1 on d: accept with probability
    min(1, p(d) / 1) = p(d), and the residual max(0, p - q) renormalised is the target with d removed - which is what
    Gumbel-max with d at -inf draws - so every out[b, 0] (and every emitted token, given its prefix) is distributed
    exactly as the target model's softmax(logits / T).

    uniform_samples float32 [B, K] in [0, 1) and gumbel_noise float32 [B * (K + 1), V]: together (the call is then
    deterministic) or not at all; absent, both are drawn from Philox keyed by ``seed`` (> 0) under fused_sampler's
    launch-offset rule, the uniform from a counter no Gumbel draw can take.  output_token_ids int32 [B, K + 1] and
    num_accepted int32 [B], when given, are written and returned as the same objects.  B == 0 returns empty tensors
    without a launch; B * (K + 1) <= 65535.  There is no host sync.
    Returns (output_token_ids, num_accepted)."""
    temp_tensor, temp_scalar = (temperature, 0.0) if isinstance(temperature, Tensor) else (None, float(temperature))
    out, acc = torch.ops.hpc_spec.speculative_verify(logits, draft_token_ids, temp_tensor, temp_scalar, uniform_samples,
                                                     gumbel_noise, seed, output_token_ids, num_accepted)
    return (out if output_token_ids is None else output_token_ids, acc if num_accepted is None else num_accepted)


@torch.library.register_fake("hpc_spec::speculative_verify")
def _speculative_verify_fake(logits, draft_token_ids, temperature, temperature_val, uniform_samples=None, gumbel_noise=None,
                             seed=0, output_token_ids=None, num_accepted=None):
    b, k = draft_token_ids.shape
    return (torch.empty((b, k + 1), dtype=torch.int32, device=logits.device),
            torch.empty((b,), dtype=torch.int32, device=logits.device))


def token_logprobs(
    logits: Tensor,
    token_ids: Tensor,
    temperature: Union[Tensor, float] = 1.0,
    num_top: int = 0,
    token_logprobs: Optional[Tensor] = None,
    token_ranks: Optional[Tensor] = None,
    top_ids: Optional[Tensor] = None,
    top_logprobs: Optional[Tensor] = None,
) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The log-probability of the token each logits row emitted, its rank, and the row's ``num_top`` most likely tokens
    with their log-probabilities, in one pass over the logits: the ``logprobs`` / ``top_logprobs`` of a completion API,
    the per-token logprobs of an RL rollout, ``prompt_logprobs`` over a prefill chunk.  It reads the logits
    fused_sampler or speculative_verify has just read and takes what they return as it is.  No reference counterpart
    (torch.ops.hpc_logprobs.token_logprobs); semantics = PyTorch (tests/token_logprobs_ref.py).

    logits [R, V] float32 / bfloat16 (inner stride 1, row stride >= V, V % 8 == 0, V < 2^20, never written).  token_ids
    int32 or int64, contiguous, R elements in any shape: [R], the [R, 1] fused_sampler returns, the [B, K + 1]
    speculative_verify returns for logits [B * (K + 1), V]; there is no cast and no host sync.  An entry < 0 or >= V marks
    a dead row (the -1 entries of a speculative step): its logits are not read and its outputs are 0.0, 0, -1 ..., 0.0 ....
    temperature: scalar >= 0, or a float32 tensor of C elements with R % C == 0, row r using entry r // (R / C) - C == R
    is a value per row, C == B the per-request tensor speculative_verify takes.  With x = logits[r].float():
        T > 0:  y = x / T (an fp32 division, speculative_verify's expression)
        T == 0: y = x, the raw distribution of a greedy request          (negative or NaN T: unspecified)
    Per row r with token t:
        token_logprobs[r] = y[t] - logsumexp(y)                                                    float32 [R]
        token_ranks[r]    = 1 + #{i : x[i] > x[t] or (x[i] == x[t] and i < t)}                     int32 [R]
        top_ids[r], top_logprobs[r] = the first num_top ids of that order, y[id] - logsumexp(y)    int32 / float32 [R, num_top]
    The order is that of the raw logits as floats - -0.0 == +0.0, ties to the smaller id: torch.sort(x, descending=True,
    stable=True) - so neither rank nor ids depend on the temperature.  Wherever rank <= num_top, top_ids[r, rank - 1] == t
    and top_logprobs[r, rank - 1] is bit-identical to token_logprobs[r].  0 <= num_top <= 32, num_top <= V; num_top == 0
    returns [R, 0] tensors and selects nothing.

    -inf logits (a masked vocabulary) are ordinary inputs: they add nothing to the sum and rank last, and a token whose
    logit is -inf has logprob -inf.  A row with a NaN, a +inf or a maximum of -inf is unspecified.

    token_logprobs, token_ranks, top_ids and top_logprobs, when given, are written and returned as the same objects.
    R == 0 returns empty tensors without a launch; any R is accepted (one launch pair per 65535 rows).  There is no host
    sync, and scratch comes from the caching allocator, so the call can be captured in a hipGraph.
    Returns (token_logprobs, token_ranks, top_ids, top_logprobs)."""
    temp_tensor, temp_scalar = (temperature, 0.0) if isinstance(temperature, Tensor) else (None, float(temperature))
    given = (token_logprobs, token_ranks, top_ids, top_logprobs)
    outs = torch.ops.hpc_logprobs.token_logprobs(logits, token_ids, temp_tensor, temp_scalar, int(num_top), *given)
    return tuple(o if g is None else g for o, g in zip(outs, given))


@torch.library.register_fake("hpc_logprobs::token_logprobs")
def _token_logprobs_fake(logits, token_ids, temperature, temperature_val, num_top, token_logprobs=None, token_ranks=None,
                         top_ids=None, top_logprobs=None):
    r, dev = logits.shape[0], logits.device
    return (torch.empty((r,), dtype=torch.float32, device=dev), torch.empty((r,), dtype=torch.int32, device=dev),
            torch.empty((r, num_top), dtype=torch.int32, device=dev), torch.empty((r, num_top), dtype=torch.float32, device=dev))
