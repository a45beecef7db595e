"""rope_norm_store_kv / rope_norm_store_kv_fp8 against the float64 statement of the op (oracle/rope.py::rope_norm_ref64)
on the bar of one rounding plus fp32 slack (tests/utils.py::rope_close), with constructed inputs (tests/rope_cases.py):
positions up to 8192+, every page edge, rows of scale 1e-3, guard pages.  Every byte of both caches is accounted for:
new tokens on the bar, cleared tails zero, all else as before the call.  tests/test_rope_bar.py shows on the CPU that
these checks reject a wrong epsilon, a sine of the wrong sign, a position off by one and the like.

Both kernel forms are covered: the narrow one (one group of eight heads per wave) by the small batches, the wide one (two
groups per wave, from 16384 (row, group) units on: what the benchmark's prefill chunk runs) by batches that assert they
reach it."""
import itertools
from types import SimpleNamespace

import pytest
import torch

import rope_cases as rc

DEVICE = "cuda"
MODES = {
    "bf16": dict(fp8=False),
    "fp8_dynamic": dict(fp8=True, quant_policy=1, k_scale=0.1, v_scale=0.07),
    "fp8_static": dict(fp8=True, quant_policy=2, k_scale=0.1, v_scale=0.07, q_scale_inv=0.3),
}
# 3, 9, 10 and 24 heads: a partial group, Q / K / V boundaries inside a group, a ragged last group
HEADS = [(1, 1), (5, 2), (8, 1), (16, 4)]
BATCHES = ["prefill"] + [f"decode-mtp{m}-req{n}" for m in (0, 1, 3) for n in (7, 16)]


def run_and_check(case, policy, is_prefill, label, fp8, quant_policy=None, k_scale=None, v_scale=None, q_scale_inv=None,
                  upper_max=None, bypass=False, wide=False):
    """one call of the op on the case, then every check of rope_cases.check_outputs on what came back"""
    import hpc

    c = case
    assert rc.is_wide(c.rows, c.hq + 2 * c.hkv) == wide, (c.rows, c.hq, c.hkv)
    dev = DEVICE
    kd, vd = rc.fresh_caches(c, fp8, dev)
    if c.buf is not None:
        assert kd.stride(0) == vd.stride(0) == 2 * c.P * c.hkv * 128
    k0, v0 = kd.cpu(), vd.cpu()
    out = SimpleNamespace(q_scale=None, flag=None, out_k=None, out_v=None)
    ok = ov = None
    if bypass:
        ok = torch.zeros(c.rows, c.hkv, 128, dtype=kd.dtype, device=dev)
        ov = torch.zeros_like(ok)
    common = (c.qkv.to(dev), c.cos_sin.to(dev), c.ns.to(dev), c.q_index.to(dev), c.ki.to(dev), is_prefill)
    norm = dict(q_norm_weight=c.qw.to(dev) if policy else None, k_norm_weight=c.kw.to(dev) if policy else None,
                qk_norm_policy=policy, out_k=ok, out_v=ov)
    scales = {}
    if fp8:
        scales = dict(k_scale=torch.tensor([k_scale]), v_scale=torch.tensor([v_scale]), quant_policy=quant_policy,
                      q_scale_inv=None if q_scale_inv is None else torch.tensor([q_scale_inv]))
        q, qs, flag = hpc.rope_norm_store_kv_fp8(
            kd, vd, *common, scales["k_scale"].to(dev), scales["v_scale"].to(dev), quant_policy,
            c.max_new, upper_max=upper_max, q_scale_inv=None if q_scale_inv is None else scales["q_scale_inv"].to(dev), **norm)
        assert flag.shape == (c.ns.shape[0], c.hkv) and flag.dtype == torch.int32
        assert (qs is None) == (quant_policy == 2)
        if qs is not None:
            assert qs.shape == ((c.ns.shape[0], c.hq, (c.max_new + 127) // 128 * 128) if is_prefill else (c.rows, c.hq))
            out.q_scale = qs.cpu()
        out.flag = flag.cpu()
    else:
        q = hpc.rope_norm_store_kv(kd, vd, *common, **norm)
    assert q.shape == (c.rows, c.hq, 128)
    out.q, out.kc, out.vc = q.cpu(), kd.cpu(), vd.cpu()
    if bypass:
        out.out_k, out.out_v = ok.cpu(), ov.cpu()
    failed = rc.check_outputs(c, policy, out, (k0, v0), fp8, upper_max=448.0 if upper_max is None else upper_max,
                              bypass=bypass, is_prefill=is_prefill, label=label, **scales)
    assert not failed, failed


def narrow_batch(batch, hq, hkv, P, interleaved=False):
    if batch == "prefill":
        return rc.prefill_case(hq, hkv, P, interleaved), True
    _, mtp, num_req = batch.split("-")
    return rc.decode_case(hq, hkv, P, int(num_req[3:]), int(mtp[3:]), interleaved), False


# the mode and the norm policy vary fastest: the cases of one batch follow each other and share its inputs and reference
@pytest.mark.gpu
@pytest.mark.parametrize("batch,heads,P,policy,mode", list(itertools.product(BATCHES, HEADS, [16, 64, 256], [0, 1, 2], MODES)),
                         ids=lambda v: f"{v[0]}q{v[1]}kv" if isinstance(v, tuple) else str(v))
def test_rope_narrow_form(batch, heads, P, policy, mode):
    case, is_prefill = narrow_batch(batch, *heads, P)
    run_and_check(case, policy, is_prefill, f"{batch} {heads} P{P} p{policy} {mode}", **MODES[mode])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("heads,rows", [((5, 2), 8192), ((8, 1), 8192), ((16, 4), 5462)], ids=["5q2kv", "8q1kv", "16q4kv"])
def test_rope_wide_form_prefill(heads, rows, mode):
    """two groups of eight heads per wave: at 9 and 10 heads the second group is ragged, at 24 heads the second unit's
    second group is past the end entirely.  Six requests share the rows unevenly."""
    run_and_check(rc.wide_prefill_case(*heads, rows), 1, True, f"wide prefill {heads} {mode}", wide=True, **MODES[mode])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_rope_wide_form_decode(mode):
    """832 requests x 2 new tokens at 64 + 2 x 8 heads (10 groups): 1664 rows reach the wide form; block size 16, so that
    the pages of the new tokens stay below 128 MB per cache"""
    case = rc.wide_decode_case(64, 8, 832, 1, 16)
    assert case.kc.numel() * 2 < 128 << 20
    run_and_check(case, 1, False, f"wide decode {mode}", wide=True, **MODES[mode])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("batch,heads,P", [("prefill", (5, 2), 64), ("decode-mtp1-req7", (16, 4), 16)])
def test_rope_interleaved_cache(batch, heads, P, mode):
    """K and V as the two halves of one [blocks, 2, P, Hkv, 128] allocation: block stride 2 * P * Hkv * 128"""
    case, is_prefill = narrow_batch(batch, *heads, P, interleaved=True)
    run_and_check(case, 2, is_prefill, f"interleaved {batch} {mode}", **MODES[mode])


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["prefill", "decode-mtp1-req7"])
def test_rope_fp8_upper_max_224(batch):
    """dynamic q scale = amax / 224 and the largest |code| of every head is 224"""
    case, is_prefill = narrow_batch(batch, 8, 1, 64)
    run_and_check(case, 1, is_prefill, f"upper_max 224 {batch}", upper_max=224.0, **MODES["fp8_dynamic"])


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["prefill", "decode-mtp3-req16"])
def test_rope_fp8_cache_saturates(batch):
    """k_scale = v_scale = 0.004: a visible share of K and V lies above 448 after scaling and must come out as +-448"""
    case, is_prefill = narrow_batch(batch, 5, 2, 16)
    ref = rc.reference(case, 1)
    live = ref.req >= 0
    for x in (ref.k64[live], ref.v[live].double()):
        assert float((x.abs() / 0.004 > 448).double().mean()) > 0.01
    run_and_check(case, 1, is_prefill, f"saturating {batch}", **dict(MODES["fp8_static"], k_scale=0.004, v_scale=0.004))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("batch", ["prefill", "decode-mtp1-req7"])
def test_rope_bypass(batch, mode):
    """out_k / out_v given: the caches stay byte-identical (no tail is cleared either), K / V land in [rows, Hkv, 128] on
    the bar, split_k_flag is zeroed all the same"""
    case, is_prefill = narrow_batch(batch, 5, 2, 64)
    run_and_check(case, 1, is_prefill, f"bypass {batch} {mode}", bypass=True, **MODES[mode])
