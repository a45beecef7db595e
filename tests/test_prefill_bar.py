"""CPU: the prefill-attention bar (tests/utils.py::attn_close on tests/prefill_needles.py inputs) and where its tau comes
from.

* the by-kv-head, q-chunked oracle used for long requests is bit-equal to the pinned oracles (block mask, per-token K
  scales, contiguous K / V included);
* on needle inputs no (token, head) row is left out of the bar and every row of the reference has max |ref| >= 0.1;
* the online model of the kernels' arithmetic stays within tau of the oracle at stages of 64 and 128 tokens over the
  cases the kernels are run on, and tau is at most 3 x the model's worst disagreement (the bar is not inflated);
* every mutant of a plausible kernel bug - the model / the oracle run on altered inputs - is >= 3 tau off;
* the reference tests' generator with their atol 0.1 accepts an all-zero answer, attn_close at that generator's tau
  does not."""
import functools

import pytest
import torch

import prefill_needles as pn
from utils import ATTN_FLOOR, allclose, attn_close, attn_rel_err

STAGES = (64, 128)


@pytest.mark.parametrize("kind,k_per_token,case", [("fp8", False, "edges_g4"), ("fp8", True, "edges_g2"), ("fp8", False, "sparse_g4"),
                                                   ("fp8", True, "sparse_g8"), ("bf16", False, "edges_g8"),
                                                   ("bf16c", False, "edges_g16")])
def test_by_kv_head_prefill_oracle_equals_pinned_oracle(kind, k_per_token, case):
    from oracle import attention as oattn

    inp = pn.case_inputs(case, kind, k_per_token, seed=2)
    a = pn.oracle(inp, pinned=True)
    assert torch.equal(a, pn.oracle(inp))
    if kind == "fp8":  # q chunks that cut requests and 128-row mask tiles
        b = oattn.ref_prefill_by_kv_head(inp["q"], inp["k"], inp["v"], inp["cu"], inp["block_ids"], inp["lens"], inp["qscale"],
                                         inp["kscale"], inp["vscale"], k_per_token, inp["block_mask"], q_chunk=37)
    else:
        # bf16: the BLAS sums P V in another order at another row count - at most one bf16 ulp of the row's scale
        b = oattn.ref_prefill_by_kv_head(inp["q"], inp["k"], inp["v"], inp["cu"], inp["block_ids"], inp["lens"], q_chunk=37)
        assert float(attn_rel_err(a, b).max()) <= 2.0 ** -7
        return
    assert torch.equal(a, b)


def test_by_kv_head_prefill_oracle_equals_pinned_oracle_on_the_reference_generator():
    for kind, ktok in (("fp8", False), ("fp8", True), ("bf16", False)):
        inp = pn.uniform_inputs(kind, [1, 37, 128, 300, 5, 64], [1, 37, 500, 300, 1000, 65], (2, 8), 32, ktok, seed=7)
        assert torch.equal(pn.oracle(inp, pinned=True), pn.oracle(inp))


@functools.lru_cache(maxsize=None)
def _needle_case(name, kind, k_per_token):
    inp = pn.case_inputs(name, kind, k_per_token)
    return inp, pn.oracle(inp)


def _uniform_cases(kind, k_per_token):
    from test_attention_prefill_fp8 import block_sparse_mask

    if kind == "bf16":  # the shapes of tests/test_attention_prefill_bf16.py
        yield pn.uniform_inputs("bf16", [500] * 2, [3000] * 2, (1, 4), 64, seed=41)
        yield pn.uniform_inputs("bf16", [1, 37, 128, 300, 5, 64], [1, 37, 500, 300, 1000, 65], (4, 32), 16, seed=7)
        yield pn.uniform_inputs("bf16c", [3907, 100, 1, 17, 64, 65], None, (2, 16), 1, seed=41)
        return
    if k_per_token:  # tests/test_attention_prefill_fp8.py::test_prefill_fp8_k_per_token
        yield pn.uniform_inputs("fp8", [200, 1, 64, 333], [700, 90, 64, 333], (1, 8), 32, True, seed=11)
        yield pn.uniform_inputs("fp8", [200, 1, 64, 333], [700, 90, 64, 333], (4, 16), 64, True, seed=11)
        return
    yield pn.uniform_inputs("fp8", [500] * 2, [3904] * 2, (1, 4), 64)
    yield pn.uniform_inputs("fp8", [1, 37, 128, 300, 5, 64], [1, 37, 500, 300, 1000, 65], (4, 32), 16, seed=7)
    for skip, heads in ((0.5, (1, 4)), (0.9, (2, 32))):  # test_blocksparse_prefill_fp8
        inp = pn.uniform_inputs("fp8", [1024] * 2, [1024] * 2, heads, 64, seed=21)
        inp["block_mask"] = block_sparse_mask(2, heads[1], 8, 8, skip, torch.Generator().manual_seed(4))
        yield inp


@pytest.mark.parametrize("generator", ["needle_fp8", "needle_fp8_ktok", "needle_bf16", "uniform_fp8", "uniform_fp8_ktok",
                                       "uniform_bf16"])
def test_online_model_within_tau(generator):
    """the online model passes attn_close at stages of 64 and 128 tokens (worst over both and over all cases <= tau), and
    tau <= 3 x that worst case; on needle inputs every row counts and every row's scale is >= 0.1"""
    needle, ktok = generator.startswith("needle"), generator.endswith("ktok")
    kind = "bf16" if generator.endswith("bf16") else "fp8"
    if needle:
        names = [n for n in pn.BAR_CASES if kind == "fp8" or not n.startswith("sparse")]
        if ktok:  # per-token K scales: pages of 32 and 64 tokens
            names = [n for n in names if pn.BAR_CASES[n][3] >= 32]
        cases = [(n, kind) + _needle_case(n, kind, ktok) for n in names]
        if kind == "bf16":
            cases += [(n, "bf16c") + _needle_case(n, "bf16c", False) for n in ("edges_g4", "edges_g16", "full_4k")]
        tau = pn.needle_tau(kind, ktok)
    else:
        cases = [("uniform %d" % i, inp["kind"], inp, pn.oracle(inp)) for i, inp in enumerate(_uniform_cases(kind, ktok))]
        tau = pn.TAU_PREFILL_UNIFORM_BF16 if kind == "bf16" else pn.TAU_PREFILL_UNIFORM_FP8_KTOK if ktok else pn.TAU_PREFILL_UNIFORM_FP8
    worst, min_scale = 0.0, float("inf")
    for name, knd, inp, ref in cases:
        scale = ref.float().abs().amax(-1)
        assert scale.shape == (int(inp["seq_q"].sum()), inp["heads"][1])
        for T in STAGES:
            rel = attn_rel_err(ref, pn.online_model(inp, T))
            assert rel.numel() == scale.numel()  # no row is left out of the bar
            w = float(rel.max())
            print(f"  {generator} {name} {knd} stage {T}: model worst {w:.4f}, row scale min {float(scale.min()):.3g}")
            worst = max(worst, w)
        min_scale = min(min_scale, float(scale.min()))
    print(f"\n{generator}: online model worst {worst:.4f} over stages {STAGES}; tau {tau} = {tau / worst:.2f} x; "
          f"smallest row scale {min_scale:.3g}")
    assert worst <= tau, (worst, tau)
    assert tau <= 3 * worst, (worst, tau)
    if needle:
        assert min_scale >= 0.1, min_scale  # ATTN_FLOOR never comes into play
    assert min_scale > ATTN_FLOOR
    assert attn_close(cases[0][3], cases[0][3].clone(), 0.0)


def _report(ref, mutants, tau, good):
    assert attn_close(ref, good, tau, label="the correct online model")
    short = []
    for name, y in mutants.items():
        m = float(attn_rel_err(ref, y).max()) / tau
        print(f"  {name:58s} {m:9.1f} tau")
        if not m >= 3:
            short.append((name, m))
    assert not short, short


@pytest.mark.parametrize("kind,k_per_token", [("fp8", False), ("fp8", True), ("bf16", False)])
def test_prefill_needle_bar_rejects_mutants(kind, k_per_token):
    """each mutant's worst (token, head) row is >= 3 tau off; the correct online model is within tau.  Requests with and
    without a cached prefix, one longer than 1024 tokens."""
    seq_q, past = [1, 37, 128, 300, 5, 64, 200, 130], [0, 0, 372, 0, 995, 1, 1100, 70]
    Hkv, Hq = heads = (2, 16)
    G = Hq // Hkv
    inp = pn.needle_inputs(seq_q, past, 64, heads, kind, k_per_token, seed=5)
    ref = pn.oracle(inp, pinned=True)
    cu, total = inp["cu"], int(inp["cu"][-1])
    bids = inp["block_ids"].clone()
    b_long = int(torch.argmax(inp["lens"]))
    bids[b_long, 1] = inp["block_ids"][(b_long + 1) % len(seq_q), 0]  # one page id replaced by another used page
    q_next = inp["q"].clone()  # request b's q rows read at cu_seqlens_q[b + 1]
    for b in range(len(seq_q)):
        idx = (int(cu[b + 1]) + torch.arange(seq_q[b])) % total
        q_next[int(cu[b]): int(cu[b + 1])] = inp["q"][idx]
    nf = lambda pa: 64 * ((pa + 1) >> 6)  # noqa: E731  first tile that is not full for the first wave of a request
    model = lambda **kw: pn.online_model(inp, 128, **kw)  # noqa: E731
    mutants = {
        "zeros": torch.zeros_like(ref),
        "x 1.25": (ref.float() * 1.25).to(ref.dtype),
        "causal limit +1": model(causal_shift=1),
        "causal limit -1": model(causal_shift=-1),
        "first token dropped": model(drop=lambda L, pa: [0]),
        "last cached token (past - 1) dropped": model(drop=lambda L, pa: [pa - 1] if pa else []),
        "64-token tile dropped at the ntile_full boundary": model(drop=lambda L, pa: list(range(nf(pa), min(L, nf(pa) + 64)))),
        "one page id swapped for another used page": model(block_ids=bids),
        "kv head h + 1 for h": model(kv_head_map=[(g + 1) % Hkv for g in range(Hkv)]),
        "q heads of one kv head rotated by one": model(q_head_map=[h - h % G + (h + 1) % G for h in range(Hq)]),
        "q rows of request b read at cu_seqlens_q[b + 1]": pn.oracle(inp, q=q_next),
    }
    if kind == "fp8":
        mutants.update({
            "qscale at position + 1": model(qscale_index=lambda b, h, p: (b, h, p + 1)),
            "qscale at head + 1": model(qscale_index=lambda b, h, p: (b, h + 1, p)),
            "qscale of request b + 1": model(qscale_index=lambda b, h, p: (b + 1, h, p)),
            "qscale indexed by the global token": model(qscale_index=lambda b, h, p: (b, h, int(cu[b]) + p)),
        })
    if k_per_token:
        mutants["K scale of token j + 1"] = model(kscale_shift=1)
        mutants["V scale of kv head h + 1"] = model(vscale_head_map=[(g + 1) % Hkv for g in range(Hkv)])
    tau = pn.needle_tau(kind, k_per_token)
    print(f"\n{kind} k_per_token={k_per_token}: tau {tau}")
    _report(ref, mutants, tau, model())


@pytest.mark.parametrize("case", ["sparse_g4", "sparse_g16"])
def test_prefill_blocksparse_bar_rejects_mutants(case):
    """the block mask's mutants, on ragged requests whose cached prefixes are not multiples of 128"""
    inp = pn.case_inputs(case, "fp8", seed=9)
    Hkv, Hq = inp["heads"]
    assert any(int(p) % 128 for p in inp["past"])
    ref = pn.oracle(inp, pinned=True)
    model = lambda **kw: pn.online_model(inp, 128, **kw)  # noqa: E731
    mutants = {
        "mask ignored": model(block_mask=None),
        "mask of q head h + 1": model(mask_head_map=[(h + 1) % Hq for h in range(Hq)]),
        "mask row r + 1": model(mask_row_shift=1),
        "mask column c + 1": model(mask_col_shift=1),
        "mask columns counted from the first q token": model(mask_from_q0=True),
        "only the first 64-token half of a column honoured": model(mask_first_half_only=True),
    }
    if Hq // Hkv == 16:
        mutants["tile skipped when any one head's bit is off"] = model(mask_any_head_off=True)
    tau = pn.TAU_PREFILL_NEEDLE_FP8
    print(f"\n{case}: tau {tau}")
    _report(ref, mutants, tau, model())


def test_reference_generator_accepts_zeros_at_reference_atol_prefill():
    """why this bar exists: on the reference grid's shape (num_seq_q 500, kv 3904, 4 / 1 heads) the literal atol 0.1
    accepts an all-zero output; attn_close at the generator's tau rejects zeros and x 1.25"""
    inp = pn.uniform_inputs("fp8", [500] * 2, [3904] * 2, (1, 4), 64)
    ref = pn.oracle(inp, pinned=True)
    zeros = torch.zeros_like(ref)
    assert allclose(ref, zeros, atol=0.1, rtol=0.02)
    assert not attn_close(ref, zeros, pn.TAU_PREFILL_UNIFORM_FP8)
    assert float(attn_rel_err(ref, (ref.float() * 1.25).to(ref.dtype)).max()) > pn.TAU_PREFILL_UNIFORM_FP8 * 1.5
    inp = pn.uniform_inputs("bf16", [500] * 2, [3000] * 2, (1, 4), 64, seed=41)
    ref = pn.oracle(inp, pinned=True)
    assert not attn_close(ref, torch.zeros_like(ref), pn.TAU_PREFILL_UNIFORM_BF16)
    assert float(attn_rel_err(ref, (ref.float() * 1.25).to(ref.dtype)).max()) > pn.TAU_PREFILL_UNIFORM_BF16 * 3
