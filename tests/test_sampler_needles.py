"""fused_sampler against planted-noise probes (tests/sampler_needles.py): every row of a batch asks one yes/no question
about the kept set, a candidate's score or the top-p cut, and the returned token is the answer.  Token equality with the
oracle (oracle/sampler.py) is exact; each case is one hpc.fused_sampler call.  What the probes are worth, and the margin
their inputs keep, is measured on the CPU by tests/test_sampler_bar.py.

    V        path of csrc/sampler.hip it reaches
    24       fewer real tokens than max_topk: padded candidates, topk > V
    264      one full 256-element segment, one of 8 elements (fewer than max_topk), 14 empty ones
    1024     4 full segments, 12 empty
    8200     768-element segments, a ragged last one, empty ones after it
    120832,  the product shapes, 16 and 19 segments: membership probes and the topk sweep only
    151936
"""
import pytest
import torch

import sampler_needles as sn
from oracle import sampler as orc

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _dev(x):
    return x.cuda() if isinstance(x, torch.Tensor) else x


def _run(case, dtype, pad=0):
    """one fused_sampler call on the case -> (tokens, mask after the call or None), both on the CPU"""
    import hpc

    logits = case["logits"].to(dtype)
    assert torch.equal(logits.float(), case["logits"])  # bf16-exact rows: both dtypes carry the same numbers
    if pad:
        wide = torch.full((case["B"], case["V"] + pad), float("inf"), dtype=dtype)
        wide[:, : case["V"]] = logits
        dev = wide.cuda()[:, : case["V"]]
        assert dev.stride(0) == case["V"] + pad and not dev.is_contiguous()
    else:
        dev = logits.cuda()
    kw = {k: _dev(v) for k, v in sn.sampler_kwargs(case).items()}
    if kw["penalty_mask"] is not None:
        kw["penalty_mask"] = case["penalty_mask"].clone().cuda()
    kw["softmax_policy"] = hpc.SoftmaxPolicy(kw["softmax_policy"])
    tok = hpc.fused_sampler(dev, **kw)
    assert tok.shape == (case["B"], 1) and tok.dtype == torch.int32
    return tok.cpu(), None if kw["penalty_mask"] is None else kw["penalty_mask"].cpu()


def _check(case, dtype, pad=0):
    tok, mask = _run(case, dtype, pad)
    ref, ref_mask = sn.oracle_answer(case)
    assert torch.equal(ref, case["expect"]), case["name"]  # the probe asks what it means to ask
    bad = (tok != ref).flatten().nonzero().flatten().tolist()
    assert not bad, [(case["name"], b, case["what"][b], "got", int(tok[b]), "oracle", int(ref[b])) for b in bad[:8]]
    if ref_mask is not None:
        assert torch.equal(mask, ref_mask), (case["name"], "penalty write-back")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("max_topk", sn.MAX_TOPK)
@pytest.mark.parametrize("V", sn.SMALL_V)
def test_probe_batches(V, max_topk, dtype):
    """membership, two-sided score and two-sided top-p probes: both logits families, the seven configurations"""
    for family in "AB":
        for ci in range(len(sn.CONFIGS)):
            _check(sn.probe_case(V, max_topk, family, ci), DTYPES[dtype])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("max_topk", sn.MAX_TOPK)
@pytest.mark.parametrize("V", sn.SMALL_V)
def test_topk_sweep(V, max_topk, dtype):
    """per-row topk 1 .. max_topk: int32 without softmax, int64 with policy 1 and a scalar topp"""
    for which in (0, 1):
        _check(sn.sweep_case(V, max_topk, which), DTYPES[dtype])


@pytest.mark.gpu
@pytest.mark.parametrize("V,max_topk,which,dtype", [(120832, 32, 1, "bf16"), (151936, 64, 0, "fp32")])
def test_product_shapes(V, max_topk, which, dtype):
    _check(sn.sweep_case(V, max_topk, which, True), DTYPES[dtype])


@pytest.mark.gpu
def test_padded_row_stride():
    """row stride V + 8 with +inf in the padding, which no segment may read"""
    _check(sn.probe_case(8200, 32, "A", 5), torch.float32, pad=8)
    _check(sn.probe_case(264, 64, "B", 3), torch.bfloat16, pad=8)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_masked_segments_policy1(dtype):
    """whole leading, trailing and middle segments at -inf under softmax-before-topk: the kept set and the top-p cut"""
    case = sn.masked_segments_case()
    _check(case, DTYPES[dtype])
    assert bool(torch.isfinite(case["logits"].gather(1, case["expect"].long())).all())


@pytest.mark.gpu
def test_penalty_writeback_bytes():
    """mask rows of 1025 bytes (not 4-byte aligned): token V - 1 in slot max_bs - 1, tokens 8k and 8k + 7, and the whole
    mask after the call"""
    case = sn.writeback_case()
    assert case["penalty_mask"].shape[1] == 1025 and int(case["slot_id"][0]) == case["penalty_mask"].shape[0] - 1
    _check(case, torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("V", [8200, 120832])
def test_fast_path_segment_edges(V, dtype):
    """temperature fast path: the arg-max at the first and last element of every (unrounded) segment and at V - 1;
    with the winner as the row's draft the runner-up across the boundary wins"""
    import hpc

    case = sn.fast_path_case(V)
    logits = case["logits"].to(DTYPES[dtype])
    dl, dt, dg = logits.cuda(), case["temperature"].cuda(), case["gumbel_noise"].cuda()
    for draft, want in ((None, case["winner"]), (case["winner"].flatten().long(), case["runner"])):
        ref = orc.ref_temperature_sample(logits, case["temperature"], case["gumbel_noise"], draft)
        assert torch.equal(ref, want)
        out = hpc.fused_sampler(dl, temperature=dt, gumbel_noise=dg, draft_token_ids=None if draft is None else draft.cuda())
        assert torch.equal(out.cpu(), ref), (out.flatten().tolist(), ref.flatten().tolist())


@pytest.mark.gpu
def test_own_noise_stays_in_the_kept_set():
    """Self-drawn Philox noise on the top-k path (policy 2, topk 8, a topp that keeps 5 or 6 tokens), 2000 launches: no
    token outside the oracle's kept set ever appears (exact), and the frequencies are within total variation 0.1 of the
    kept set's renormalised probabilities - the bar of test_sampler.py::test_temperature_distribution, about 5 x the
    sampling noise at this N; a sampler that ignores its noise sits above 0.5."""
    import hpc

    case = sn.own_noise_case()
    B, V, N = case["B"], case["V"], 2000
    dev = case["logits"].cuda()
    kw = dict(case["kwargs"])
    kw["softmax_policy"] = hpc.SoftmaxPolicy(kw["softmax_policy"])
    counts = torch.zeros(B, V, device="cuda")
    for _ in range(N):
        tok = hpc.fused_sampler(dev, seed=42, **kw)
        counts.scatter_add_(1, tok.to(torch.int64), torch.ones_like(tok, dtype=torch.float32))
    counts = counts.cpu()
    want = torch.zeros(B, V, dtype=torch.float64)
    for b in range(B):
        for t, p in case["kept"][b].items():
            want[b, t] = p
    assert int(counts[want == 0].sum()) == 0, "a token outside the kept set was sampled"
    tv = 0.5 * (counts.double() / N - want).abs().sum(dim=-1)
    print("total variation per row:", tv.tolist())
    assert (tv < 0.1).all(), tv.tolist()
