"""CPU: the decode-attention bar (tests/utils.py::attn_close) and where its tau comes from (tests/decode_needles.py).

* the per-kv-head oracle used for long requests is bit-equal to the pinned oracles;
* the split-K model of the kernels' arithmetic stays within tau of the oracle at every range length 16 ... 4096, and
  tau is at most 3 x the model's worst disagreement (the bar is not inflated);
* every mutant of a plausible kernel bug - run as the oracle / the model on altered inputs - is rejected at >= 3 tau;
* the reference tests' generator with their atol 0.2 accepts an all-zero answer (why the bar exists), while attn_close
  with that generator's tau rejects zeros and a x 1.25 scale error."""
import math

import pytest
import torch

import decode_needles as dn
from utils import ATTN_FLOOR, allclose, attn_close, attn_rel_err

F8 = torch.float8_e4m3fn


def test_attn_close_basics():
    ref = torch.randn(6, 8, 128).to(torch.bfloat16)
    ref[2, 3] = 0  # an all-zero reference row: measured against the floor
    assert attn_close(ref, ref.clone(), 1e-6, num_seq_q=2)
    bad = ref.clone()
    bad[5, 1, 7] += 0.5
    rel = attn_rel_err(ref, bad, num_seq_q=2)
    assert rel.shape == (3, 2, 8) and float(rel[2, 1, 1]) > 0.1 and int((rel > 0).sum()) == 1
    assert not attn_close(ref, bad, 0.05, num_seq_q=2)
    nan = ref.clone()
    nan[0, 0, 0] = float("nan")
    assert not attn_close(ref, nan, 1e6)
    small = ref.clone()
    small[2, 3, 0] = ATTN_FLOOR / 4  # below the floor: 0.25 of it
    assert abs(float(attn_rel_err(ref, small)[2, 0, 3]) - 0.25) < 5e-3


def _pages(lens_total, P, nblk_extra, seed):
    g = torch.Generator().manual_seed(seed)
    nblocks = (lens_total + P - 1) // P
    nblk = int(nblocks.sum()) + nblk_extra
    perm = torch.randperm(nblk, generator=g).int()
    bid = torch.zeros(len(lens_total), int(nblocks.max()), dtype=torch.int32)
    o = 0
    for i, n in enumerate(nblocks.tolist()):
        bid[i, :n] = perm[o: o + n]
        o += n
    return bid, nblocks, nblk


@pytest.mark.parametrize("k_per_token,literal", [(False, False), (True, False), (False, True)])
def test_by_kv_head_oracle_equals_pinned_fp8_oracle(k_per_token, literal):
    from oracle import attention as oattn

    torch.manual_seed(1)
    Sq, Hkv, Hq, D, P = 2, 2, 16, 128, 64
    lens_before = torch.tensor([100, 3, 700, 0], dtype=torch.int32)
    bid, nblocks, nblk = _pages(lens_before + Sq, P, 3, 1)
    rows = P * 4 // D if k_per_token else 0
    kv = torch.randn(nblk, 2, P + rows, Hkv, D)
    if k_per_token:
        kc, _ = oattn.quant_paged_cache_pertoken(kv[:, 0], P)
        kv8 = torch.empty_like(kv, dtype=F8)
        kv8[:, 0], kv8[:, 1] = kc, kv[:, 1].to(F8)
        ks, vs = kv8[:, 0, P:], torch.rand(Hkv) + 0.1
    else:
        kv8 = kv.to(F8)
        ks, vs = torch.tensor([0.3]), torch.tensor([0.7])
    q = torch.randn(4 * Sq, Hq, D).to(F8)
    qs = torch.rand(4 * Sq, Hq) * 0.1
    a = oattn.ref_attn_fp8(q, kv8[:, :, :P], bid, nblocks, Sq, lens_before, qs, ks, vs, k_per_token, literal)
    b = oattn.ref_attn_by_kv_head(q, kv8[:, :, :P], bid, Sq, lens_before + Sq, None, qs, ks, vs, k_per_token, literal)
    assert torch.equal(a.reshape(b.shape), b)
    c = oattn.ref_attn_by_kv_head(q, kv8[:, :, :P], bid, Sq, lens_before + Sq, [2, 0], qs, ks, vs, k_per_token, literal)
    assert torch.equal(c, b[[2, 0]])


def test_by_kv_head_oracle_equals_pinned_bf16_oracle():
    from oracle import attention as oattn

    torch.manual_seed(2)
    Sq, Hkv, Hq, D, P = 3, 2, 8, 128, 32
    lens_before = torch.tensor([100, 3, 700, 0], dtype=torch.int32)
    bid, nblocks, nblk = _pages(lens_before + Sq, P, 3, 2)
    kv = torch.randn(nblk, 2, P, Hkv, D, dtype=torch.bfloat16)
    q = torch.randn(4 * Sq, Hq, D, dtype=torch.bfloat16) / math.sqrt(D)
    a = oattn.ref_attn_with_paged_kvcache(q, kv, bid, nblocks, Sq, lens_before)
    b = oattn.ref_attn_by_kv_head(q, kv, bid, Sq, lens_before + Sq)
    assert torch.equal(a.reshape(b.shape), b)


# (generator, cases) -> tau: the cases the bars are calibrated on
_NEEDLE_CASES = [([0, 1, 63, 64, 1500, 4000], 2, (2, 16), 64), ([16000, 9000, 3, 1025], 1, (1, 8), 64),
                 ([5000, 700], 4, (2, 16), 64), ("edges", 2, (8, 64), 32)]
_UNIFORM_CASES = [("randint", 2, (1, 8)), ([9000, 3, 130, 65, 2049], 2, (2, 16)), ([20000, 700, 1], 4, (1, 8))]


def _uniform_lens(spec):
    if spec == "randint":
        return torch.randint(1, 4096, (6,), dtype=torch.int32, generator=torch.Generator().manual_seed(41))
    return torch.tensor(spec, dtype=torch.int32)


def _uniform_bf16(lens, Sq, heads):
    from test_attention_decode_bf16 import _build_case

    q, kvc, bid, nb = _build_case(len(lens), Sq, lens, 64, heads, "NHD")
    return dict(q=q, kv=kvc, block_ids=bid, nblocks=nb, lens_before=lens, lens_total=lens + Sq, num_seq_q=Sq, P=64,
                heads=heads, kind="bf16", k_per_token=False)


def _worst_model_error(inputs):
    worst = 0.0
    for inp in inputs:
        ref = dn.oracle(inp)
        for R in dn.RANGE_LENS:
            worst = max(worst, float(attn_rel_err(ref, dn.split_model(inp, R), inp["num_seq_q"]).max()))
    return worst


@pytest.mark.parametrize("generator", ["needle_fp8", "needle_fp8_ktok", "needle_bf16", "uniform_fp8", "uniform_fp8_ktok",
                                       "uniform_bf16"])
def test_split_model_within_tau(generator):
    """the split-K model passes attn_close at every range length (worst over all of them <= tau), and tau <= 3 x that
    worst case; the oracle passes itself exactly"""
    if generator.startswith("needle"):
        kind = "bf16" if generator.endswith("bf16") else "fp8"
        inputs = [dn.needle_inputs(dn.edge_lens(P, sq) if l == "edges" else torch.tensor(l, dtype=torch.int32), sq, P, h,
                                   kind, generator.endswith("ktok"), seed=11) for l, sq, h, P in _NEEDLE_CASES]
        tau = dn.needle_tau(kind, generator.endswith("ktok"))
    elif generator == "uniform_bf16":
        inputs = [_uniform_bf16(_uniform_lens(l), sq, h) for l, sq, h in _UNIFORM_CASES[:2]]
        tau = dn.TAU_UNIFORM_BF16
    else:
        ktok = generator.endswith("ktok")
        inputs = [dn.uniform_inputs_fp8(_uniform_lens(l), sq, 64, h, ktok) for l, sq, h in _UNIFORM_CASES]
        tau = dn.TAU_UNIFORM_FP8_KTOK if ktok else dn.TAU_UNIFORM_FP8
    worst = _worst_model_error(inputs)
    print(f"\n{generator}: split model worst {worst:.4f} over range lengths {dn.RANGE_LENS}; tau {tau} = {tau / worst:.2f} x")
    assert worst <= tau, (worst, tau)
    assert tau <= 3 * worst, (worst, tau)
    ref = dn.oracle(inputs[0])
    assert attn_close(ref, ref.clone(), 0.0, inputs[0]["num_seq_q"])


def _mutants(inp):
    """name -> the output of a plausibly wrong kernel, made by running the oracle / the model on altered inputs"""
    ref = dn.oracle(inp)
    Hkv = inp["heads"][0]
    bid = inp["block_ids"].clone()
    b_long = int(torch.argmax(inp["lens_total"]))
    b_other = next(b for b in range(len(bid)) if b != b_long and int(inp["nblocks"][b]) > 0)
    bid[b_long, 1] = inp["block_ids"][b_other, 0]  # one page id replaced by another (used) page of the pool
    out = {
        "zeros": torch.zeros_like(ref),
        "x1.25 (v_scale, 1/256)": (ref.float() * 1.25).to(ref.dtype),
        "last token dropped": dn.split_model(inp, drop=lambda L: [L - 1]),
        "first token dropped": dn.split_model(inp, drop=lambda L: [0]),
        "page id swapped": dn.split_model(inp, block_ids=bid),
        "kv head h+1 for h": dn.split_model(inp, kv_head_map=[(g + 1) % Hkv for g in range(Hkv)]),
        "causal mask +1 on new rows": dn.split_model(inp, causal_shift=1),
        "causal mask -1 on new rows": dn.split_model(inp, causal_shift=-1),
        "first split range counted twice": dn.split_model(inp, 512, range_mult=(0, 2.0)),
        "first split range left out": dn.split_model(inp, 512, range_mult=(0, 0.0)),
        "last split range counted twice": dn.split_model(inp, 512, range_mult=(-1, 2.0)),
        "last split range left out": dn.split_model(inp, 512, range_mult=(-1, 0.0)),
    }
    if inp["kind"] == "fp8":
        out["q_scale row bi (reference test's indexing)"] = dn.oracle(inp, literal_qscale_row=True)
    return ref, out


@pytest.mark.parametrize("kind,k_per_token", [("fp8", False), ("fp8", True), ("bf16", False)])
def test_needle_bar_rejects_mutants(kind, k_per_token):
    """each mutant's worst (request, row, head) is >= 3 tau off; the model at a correct split is within tau"""
    inp = dn.needle_inputs(torch.tensor([0, 1, 63, 64, 1500, 4000], dtype=torch.int32), 2, 64, (2, 16), kind, k_per_token,
                           seed=5)
    tau = dn.needle_tau(kind, k_per_token)
    ref, mutants = _mutants(inp)
    print(f"\n{kind} k_per_token={k_per_token}: tau {tau}")
    short = []
    for name, y in mutants.items():
        m = float(attn_rel_err(ref, y, 2).max()) / tau
        print(f"  {name:45s} {m:9.1f} tau")
        if not m >= 3:
            short.append((name, m))
    assert not short, short


def test_reference_generator_accepts_zeros_at_reference_atol():
    """why this bar exists: with the reference tests' generator (near-uniform softmax, |y| ~ 1e-2 ... 1e-3) the literal
    atol 0.2 / 0.1 accepts an all-zero output; attn_close at the generator's tau rejects zeros and x 1.25"""
    for ktok, atol, tau in ((False, 0.2, dn.TAU_UNIFORM_FP8), (True, 0.1, dn.TAU_UNIFORM_FP8_KTOK)):
        inp = dn.uniform_inputs_fp8(torch.tensor([4095, 1000, 130], dtype=torch.int32), 2, 64, (1, 8), ktok)
        ref = dn.oracle(inp)
        assert allclose(ref, torch.zeros_like(ref), atol=atol)
        assert not attn_close(ref, torch.zeros_like(ref), tau, 2)
        assert float(attn_rel_err(ref, (ref.float() * 1.25).to(ref.dtype), 2).max()) > tau * 1.5
    inp = _uniform_bf16(torch.tensor([4095, 1000, 130], dtype=torch.int32), 2, (1, 8))
    ref = dn.oracle(inp)
    assert not attn_close(ref, torch.zeros_like(ref), dn.TAU_UNIFORM_BF16, 2)
    assert float(attn_rel_err(ref, (ref.float() * 1.25).to(ref.dtype), 2).max()) > dn.TAU_UNIFORM_BF16 * 3
