"""hpc.stem: Stem block-sparse mask generation (prep_paged_kv, prep_varlen_q, oam_gemm, tpd, stem_paged_kv) against the
CPU restatement in tests/stem_ref.py, its schemas / signatures / fakes against the reference's, and its mask fed to the
block-sparse FP8 prefill."""
import json
import sys
from pathlib import Path

import pytest
import torch
from torch._subclasses import FakeTensorMode

import hpc
import stem_ref as sr
from oracle import attention as oattn
from utils import allclose

GOLDEN = Path(__file__).parent / "golden"
F8, BF = torch.float8_e4m3fn, torch.bfloat16
OPS = ("stem_oam_prep_paged_kv", "stem_oam_prep_varlen_q", "stem_oam_gemm", "stem_tpd")


# ---- CPU: surface ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OPS)
def test_schema_equals_reference_in_hpc_stem_namespace(name):
    ref = json.loads((GOLDEN / "ref_schemas.json").read_text())[name]["schema"]
    ours = str(getattr(torch.ops.hpc_stem, name).default._schema)
    assert ours == str(torch._C.parse_schema("hpc_stem::" + ref))


def test_python_signatures_equal_reference():
    sys.path.insert(0, str(GOLDEN))
    from extract_schemas import py_signatures

    ref = {k: v for k, v in json.loads((GOLDEN / "ref_py_signatures.json").read_text()).items() if k.startswith("stem_")}
    ours = py_signatures(Path(hpc.__file__).parent / "stem.py")
    assert len(ref) == 5
    for name, v in ref.items():
        assert ours.get(name) == v["args"], name
        assert callable(getattr(hpc, name))


def test_fakes_give_the_reference_upper_bound_shapes():
    def T(*shape, dtype=BF):
        return torch.empty(shape, dtype=dtype, device="cuda")

    ops = torch.ops.hpc_stem
    B, Hq, Hkv, P, npages, mb = 3, 16, 2, 64, 40, 7
    with FakeTensorMode():
        kc = T(npages, P, Hkv, 128, dtype=F8)
        kf, vb = ops.stem_oam_prep_paged_kv(kc, kc, T(1, dtype=torch.float32), T(1, dtype=torch.float32),
                                            T(B, mb, dtype=torch.int32), T(B, dtype=torch.int32), 0.3, 128, 16, 1)
        max_kb = (mb * P + 127) // 128
        assert (tuple(kf.shape), kf.dtype) == ((B, Hkv, max_kb, 2048), BF)
        assert (tuple(vb.shape), vb.dtype) == ((B, Hkv, max_kb), torch.float32)
        qf = ops.stem_oam_prep_varlen_q(T(500, Hq, 128, dtype=F8), T(B, Hq, 300, dtype=torch.float32),
                                        T(B, dtype=torch.int32), T(B + 1, dtype=torch.int32), 128, 16)
        assert (tuple(qf.shape), qf.dtype) == ((B, Hq, 3, 2048), BF)
        lg = ops.stem_oam_gemm(qf, kf, vb, T(B, dtype=torch.int32), T(B, dtype=torch.int32), 128, 16, True)
        assert (tuple(lg.shape), lg.dtype) == ((B, Hq, 3, max_kb), BF)
        m = ops.stem_tpd(lg, T(B, dtype=torch.int32), T(B, dtype=torch.int32), T(B, dtype=torch.int32), 128, 1.0, 4, 4,
                         0.2, 30, 0.1, 30)
        assert (tuple(m.shape), m.dtype) == ((B, Hq, 3, max_kb), torch.uint8)


def _tricky_logits(shape, gen):
    """bf16 logits with many ties, +-0.0, NaN and -inf."""
    x = (torch.randint(-40, 41, shape, generator=gen).float() / 8).to(BF)
    u = torch.rand(shape, generator=gen)
    x[u < 0.05] = 0.0
    x[(u >= 0.05) & (u < 0.10)] = -0.0
    x[(u >= 0.10) & (u < 0.13)] = float("nan")
    x[(u >= 0.13) & (u < 0.18)] = float("-inf")
    return x


def test_oracle_threshold_equals_brute_force():
    g = torch.Generator().manual_seed(3)
    keys = sr.order_keys(_tricky_logits((40, 300), g))
    n = torch.randint(1, 301, (40,), generator=g)
    keys = torch.where(torch.arange(300)[None, :] < n[:, None], keys, torch.zeros((), dtype=torch.int32))
    budget = torch.randint(0, 320, (40,), generator=g)
    T = sr.thresholds(keys, budget)
    for i in range(40):
        fin = keys[i][keys[i] >= 0x80].sort(descending=True)[0]
        b = int(budget[i])
        want = 0x80 if b >= fin.numel() else (0xFFFF if b <= 0 else int(fin[b - 1]))
        assert int(T[i]) == want, (i, b, fin.numel())
    # the order: -0.0 below +0.0, non-finite below every finite value
    k = sr.order_keys(torch.tensor([-0.0, 0.0, float("nan"), float("-inf"), -3e38, 1.0], dtype=BF))
    assert k[0] < k[1] and k[2] == k[3] == 0x7F and 0x7F < k[4] < k[0] < k[5]


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def _close_bf16(got, ref, floor):
    """finite values within one bf16 ulp of the float64 reference, or within `floor` (broadcast) of it."""
    d = (got.double() - ref).abs()
    return bool((d <= torch.maximum(sr.bf16_ulp(ref), floor)).all())


def _paged_case(kv_lens, hkv, P, quant_type, gen, needle=None):
    """FP8 paged K / V caches with a randomly permuted page table; quant_type 0: per-token K scales in the cache's
    tail rows (oracle.attention.quant_paged_cache_pertoken) and per-head V scales."""
    B = len(kv_lens)
    npg = [sr.cdiv(L, P) for L in kv_lens]
    nblk = sum(npg) + 3
    kf = torch.randn(nblk, P, hkv, 128, generator=gen) * 0.5
    vf = torch.randn(nblk, P, hkv, 128, generator=gen) * torch.rand(nblk, P, hkv, 1, generator=gen) * 2
    perm = torch.randperm(nblk, generator=gen).to(torch.int32)
    ids = torch.zeros(B, max(npg) + 1, dtype=torch.int32)
    o = 0
    for b, n in enumerate(npg):
        ids[b, :n] = perm[o:o + n]
        o += n
    if needle is not None:  # needle(kf, ids) plants K rows
        needle(kf, ids)
    if quant_type == 1:
        kc, vc = kf.to(F8), vf.to(F8)
        ks, vs = torch.tensor([0.7]), torch.tensor([1.3])
    else:
        full = torch.cat([kf, torch.zeros(nblk, P // 32, hkv, 128)], 1)
        c8, ks = oattn.quant_paged_cache_pertoken(full, P)
        kc = c8[:, :P]
        vc, vs = oattn.quant_paged_cache_perhead(vf, P)
    return kc, vc, ks, vs, ids, torch.tensor(kv_lens, dtype=torch.int32)


def _q_case(q_lens, hq, gen, u=None):
    B = len(q_lens)
    tot = sum(q_lens)
    q = torch.randn(tot, hq, 128, generator=gen)
    if u is not None:
        q = q * 0.3 + u
    q = q.to(F8)
    pad = sr.cdiv(max(q_lens), 128) * 128 + 64
    qscale = torch.rand(B, hq, pad, generator=gen) * 0.1 + 0.02
    cu = torch.tensor([0] + list(torch.tensor(q_lens).cumsum(0)), dtype=torch.int32)
    return q, qscale, torch.tensor(q_lens, dtype=torch.int32), cu


def _cuda(*xs):
    return [x.cuda() for x in xs]


# ---- GPU: stages ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("quant_type", [0, 1])
@pytest.mark.parametrize("P", [32, 64])
def test_prep_paged_kv(quant_type, P):
    g = torch.Generator().manual_seed(11 + P + quant_type)
    kv_lens = [1000, 1, 129, 384, 2500]
    kc, vc, ks, vs, ids, lens = _paged_case(kv_lens, 2, P, quant_type, g)
    kflat, vbias = hpc.stem_oam_prep_paged_kv(*_cuda(kc, vc, ks, vs, ids, lens), 0.3, 128, 16, hpc.QuantType(quant_type))
    rk, rv = sr.prep_paged_kv(kc, vc, ks, vs, ids, lens, 0.3, quant_type)
    kflat, vbias = kflat.cpu(), vbias.cpu()
    assert kflat.shape == rk.shape and vbias.shape == rv.shape and kflat.dtype == BF
    nkb = sr.cdiv(lens, 128)
    valid = (torch.arange(rk.shape[2])[None, :] < nkb[:, None])[:, None, :].expand(rk.shape[:3])
    floor = 1e-3 * rk.abs().amax(-1, keepdim=True)
    assert _close_bf16(kflat[valid], rk[valid], floor.expand_as(rk)[valid])
    assert bool((kflat[~valid] == 0).all()) and bool((vbias[~valid] == 0).all())
    assert torch.allclose(vbias.double(), rv, atol=1e-4, rtol=1e-4)
    if quant_type == 0:  # the fp32 scale tensor and its fp8 view are the same input
        k2, v2 = hpc.stem_oam_prep_paged_kv(*_cuda(kc, vc, ks.view(torch.float32), vs, ids, lens), 0.3, 128, 16,
                                            hpc.QuantType(0))
        assert torch.equal(k2.cpu(), kflat) and torch.equal(v2.cpu(), vbias)


@pytest.mark.gpu
def test_prep_varlen_q():
    g = torch.Generator().manual_seed(5)
    q, qscale, ql, cu = _q_case([700, 1, 128, 1300], 4, g)
    qflat = hpc.stem_oam_prep_varlen_q(*_cuda(q, qscale, ql, cu)).cpu()
    ref = sr.prep_varlen_q(q, qscale, ql, cu)
    assert qflat.shape == ref.shape
    nqb = sr.cdiv(ql, 128)
    valid = (torch.arange(ref.shape[2])[None, :] < nqb[:, None])[:, None, :].expand(ref.shape[:3])
    floor = 1e-3 * ref.abs().amax(-1, keepdim=True)
    assert _close_bf16(qflat[valid], ref[valid], floor.expand_as(ref)[valid])
    assert bool((qflat[~valid] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("hkv", [8, 2, 1])
def test_oam_gemm(causal, hkv):
    g = torch.Generator().manual_seed(hkv * 2 + causal)
    hq = 8
    ql = torch.tensor([9000, 1000, 129], dtype=torch.int32)
    kl = torch.tensor([17000, 20000, 129], dtype=torch.int32)
    mq, mk = int(sr.cdiv(ql, 128).max()), int(sr.cdiv(kl, 128).max())  # 71, 157
    qflat = (torch.randn(3, hq, mq, 2048, generator=g) * 0.5).to(BF)
    kflat = (torch.randn(3, hkv, mk, 2048, generator=g) * 0.5).to(BF)
    vbias = torch.rand(3, hkv, mk, generator=g)
    got = hpc.stem_oam_gemm(*_cuda(qflat, kflat, vbias, ql, kl), causal=causal).cpu()
    ref = sr.oam_gemm(qflat, kflat, vbias, ql, kl, causal)
    assert got.shape == ref.shape and got.dtype == BF
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isneginf(got.float()), ~fin)
    floor = 1e-3 * ref.masked_fill(~fin, 0).abs().amax(-1, keepdim=True)
    assert _close_bf16(got[fin], ref[fin], floor.expand_as(ref)[fin])


TPD_CASES = {  # q_lens, kv_lens, num_prompt_tokens, alpha
    "small": ([300, 129, 1], [900, 129, 640], [900, 129, 640], 1.0),
    "medium_decay": ([5000, 37], [9000, 7000], [9000, 7000], 0.5),
    "large_chunked": ([2000, 700], [30000, 25000], [40000, 26000], 0.5),
    "kb1500": ([300], [1500 * 128 - 7], [1500 * 128 - 7], 1.0),
    "kb4200": ([260], [4200 * 128 - 100], [4200 * 128], 0.5),
    "kb9000": ([129], [9000 * 128], [9000 * 128], 1.0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(TPD_CASES))
def test_tpd_equals_oracle(case):
    q_lens, kv_lens, npt, alpha = TPD_CASES[case]
    g = torch.Generator().manual_seed(len(case))
    ql, kl, nt = (torch.tensor(x, dtype=torch.int32) for x in (q_lens, kv_lens, npt))
    H = 3
    shape = (len(q_lens), H, int(sr.cdiv(ql, 128).max()), int(sr.cdiv(kl, 128).max()))
    logits = _tricky_logits(shape, g)
    got = hpc.stem_tpd(*_cuda(logits, ql, kl, nt), alpha=alpha).cpu()
    ref = sr.tpd(logits, ql, kl, nt, alpha=alpha)
    assert got.dtype == torch.uint8 and torch.equal(got, ref), int((got != ref).sum())


# ---- GPU: end to end --------------------------------------------------------------------------------------------------
NEEDLE_BLOCK = 20
E2E_KW = dict(k_block_num_rate_medium=0.05, k_block_num_bias_medium=2)  # budget 5 of 71 blocks in the long request


def _e2e_case(quant_type, gen):
    """Every q row leans towards one direction u; the K rows of kv block NEEDLE_BLOCK are u.  Request 0 is dense
    (P < 56: the budget covers every block), request 1 is chunked (700 q tokens after 8300 cached) and sparse."""
    hq, hkv, P = 4, 2, 64
    q_lens, kv_lens = [1500, 700], [1500, 9000]
    u = torch.randn(128, generator=gen).sign()

    def plant(kf, ids):
        for b, L in enumerate(kv_lens):
            for t in range(NEEDLE_BLOCK * 128, min(NEEDLE_BLOCK * 128 + 128, L)):
                kf[ids[b, t // P].long(), t % P, :, :] = u * 1.5

    kc, vc, ks, vs, ids, kl = _paged_case(kv_lens, hkv, P, quant_type, gen, needle=plant)
    q, qscale, ql, cu = _q_case(q_lens, hq, gen, u=u)
    return q, kc, vc, qscale, ks, vs, ids, cu, kl, ql


@pytest.mark.gpu
@pytest.mark.parametrize("quant_type", [0, 1])
def test_stem_paged_kv_end_to_end(quant_type):
    g = torch.Generator().manual_seed(40 + quant_type)
    q, kc, vc, qscale, ks, vs, ids, cu, kl, ql = _e2e_case(quant_type, g)
    qt = hpc.QuantType(quant_type)
    d = _cuda(q, kc, vc, qscale, ks, vs, ids, cu, kl)
    mask = hpc.stem_paged_kv(*d, kl.cuda(), quant_type=qt, **E2E_KW)
    # the composition of the four ops
    kflat, vbias = hpc.stem_oam_prep_paged_kv(d[1], d[2], d[4], d[5], d[6], d[8], quant_type=qt)
    qflat = hpc.stem_oam_prep_varlen_q(d[0], d[3], ql.cuda(), d[7])
    lg = hpc.stem_oam_gemm(qflat, kflat, vbias, ql.cuda(), d[8])
    assert torch.equal(mask, hpc.stem_tpd(lg, ql.cuda(), d[8], kl.cuda(), **E2E_KW))
    # the oracle pipeline: float64 stages, bf16 where the kernels store bf16
    rk, rv = sr.prep_paged_kv(kc, vc, ks, vs, ids, kl, 0.3, quant_type)
    rq = sr.prep_varlen_q(q, qscale, ql, cu)
    rl = sr.oam_gemm(rq.to(BF), rk.to(BF), rv.float(), ql, kl).to(BF)
    rm, T = sr.tpd(rl, ql, kl, kl, return_threshold=True, **E2E_KW)
    mask = mask.cpu()
    assert mask.shape == rm.shape
    # fixed patterns (initial / window / diagonal) and everything outside the requests agree exactly
    off = sr.c_div(kl.long() - ql.long() + 127, 128)
    nkb, nqb = sr.cdiv(kl.long(), 128), sr.cdiv(ql.long(), 128)
    r = torch.arange(rm.shape[2])[None, None, :, None]
    c = torch.arange(rm.shape[3])[None, None, None, :]
    diag = torch.minimum(r + off[:, None, None, None], nkb[:, None, None, None] - 1)
    inside = (r < nqb[:, None, None, None]) & (c < nkb[:, None, None, None])
    fixed = (c < 4) | ((c > diag - 4) & (c <= diag))
    fixed = fixed.expand_as(rm) | ~inside.expand_as(rm)
    assert torch.equal(mask[fixed], rm[fixed])
    # every other mismatch is a near-tie with the row's threshold (within 2 bf16 ulp)
    miss = (mask != rm).nonzero().tolist()
    for b, h, i, j in miss:
        t = int(T[b, h, i])
        bits = t ^ 0x8000 if t & 0x8000 else (~t) & 0xFFFF
        thr_val = torch.tensor([bits], dtype=torch.int32).to(torch.int16).view(BF).double()[0]
        v = rl[b, h, i, j].double()
        assert abs(v - thr_val) <= 2 * sr.bf16_ulp(thr_val), (b, h, i, j, float(v), float(thr_val))
    # the needle block is selected in every row that can see it
    sees = inside & (diag >= NEEDLE_BLOCK)
    sees = sees.expand_as(mask)[:, :, :, NEEDLE_BLOCK]
    assert bool(sees.any()) and bool((mask[:, :, :, NEEDLE_BLOCK][sees] == 1).all())
    assert float(mask[1].float().mean()) < 0.5  # the long request is sparse


@pytest.mark.gpu
@pytest.mark.parametrize("quant_type", [0, 1])
def test_mask_feeds_blocksparse_prefill(quant_type):
    g = torch.Generator().manual_seed(60 + quant_type)
    q, kc, vc, qscale, ks, vs, ids, cu, kl, ql = _e2e_case(quant_type, g)
    qt = hpc.QuantType(quant_type)
    d = _cuda(q, kc, vc, qscale, ks, vs, ids, cu, kl)
    mask = hpc.stem_paged_kv(*d, kl.cuda(), quant_type=qt, **E2E_KW)
    assert 0 < int(mask.sum()) < mask.numel()
    y = hpc.attention_with_kvcache_blocksparse_prefill_fp8(d[0], d[1], d[2], d[3], d[4], d[5], d[7], d[6], d[8],
                                                           int(ql.max()), quant_type=qt, block_mask=mask)
    gt = oattn.ref_prefill_fp8(q, kc, vc, qscale, ks, vs, cu, ids, kl, k_per_token=quant_type == 0,
                               block_mask=mask.cpu())
    assert allclose(gt, y.cpu(), atol=0.1, rtol=0.02)


@pytest.mark.gpu
def test_replay_every_op():
    import replay_check as rc

    g = torch.Generator().manual_seed(77)
    q, kc, vc, qscale, ks, vs, ids, cu, kl, ql = _e2e_case(0, g)
    d = _cuda(q, kc, vc, qscale, ks, vs, ids, cu, kl)
    qt = hpc.QuantType(0)
    kflat, vbias = rc.replay_call("stem_oam_prep_paged_kv", (d[1], d[2], d[4], d[5], d[6], d[8]), {"quant_type": qt},
                                  hpc.stem_oam_prep_paged_kv)
    qflat = rc.replay_call("stem_oam_prep_varlen_q", (d[0], d[3], ql.cuda(), d[7]), {}, hpc.stem_oam_prep_varlen_q)
    lg = rc.replay_call("stem_oam_gemm", (qflat, kflat, vbias, ql.cuda(), d[8]), {}, hpc.stem_oam_gemm)
    rc.replay_call("stem_tpd", (lg, ql.cuda(), d[8], kl.cuda()), {"alpha": 0.5}, hpc.stem_tpd)


@pytest.mark.gpu
def test_refusals():
    dev = "cuda"
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
    kc = torch.zeros(4, 64, 1, 128, device=dev).to(F8)
    one = torch.ones(1, device=dev)
    ids, kl = i32([0, 1]), i32(100)
    ids = ids.view(1, 2)
    ops = torch.ops.hpc_stem
    bad = [
        lambda: ops.stem_oam_prep_paged_kv(kc, kc, one, one, ids, kl, 0.3, 64, 16, 1),            # block / stride
        lambda: ops.stem_oam_prep_paged_kv(kc, kc, one, one, ids, kl, 0.3, 128, 8, 1),
        lambda: ops.stem_oam_prep_paged_kv(kc, kc, one, one, ids, kl, 0.3, 128, 16, 2),           # quant_type
        lambda: ops.stem_oam_prep_paged_kv(kc, kc, one.double(), one, ids, kl, 0.3, 128, 16, 1),  # kscale dtype
        lambda: ops.stem_oam_prep_paged_kv(kc[:, :16], kc[:, :16], one, one, ids, kl, 0.3, 128, 16, 1),  # page 16
        lambda: ops.stem_oam_prep_paged_kv(kc[..., :64], kc[..., :64], one, one, ids, kl, 0.3, 128, 16, 1),  # dim
    ]
    q = torch.zeros(10, 2, 128, device=dev).to(F8)
    qs = torch.ones(1, 2, 128, device=dev)
    ql, cu = i32(10), i32(0, 10)
    bad += [
        lambda: ops.stem_oam_prep_varlen_q(q, qs, ql, cu, 256, 16),
        lambda: ops.stem_oam_prep_varlen_q(q[..., :64].contiguous(), qs, ql, cu, 128, 16),
        lambda: ops.stem_oam_prep_varlen_q(q, qs[0], ql, cu, 128, 16),
    ]
    qf = torch.zeros(1, 2, 1, 2048, device=dev, dtype=BF)
    kf = torch.zeros(1, 1, 1, 2048, device=dev, dtype=BF)
    vb = torch.zeros(1, 1, 1, device=dev)
    bad += [
        lambda: ops.stem_oam_gemm(qf, kf, vb, ql, kl, 128, 32, True),
        lambda: ops.stem_oam_gemm(qf[..., :1024].contiguous(), kf[..., :1024].contiguous(), vb, ql, kl, 128, 16, True),
        lambda: ops.stem_oam_gemm(qf, kf, torch.zeros(1, 1, 2, device=dev), ql, kl, 128, 16, True),
    ]
    lg = torch.zeros(1, 2, 1, 4, device=dev, dtype=BF)
    tpd = lambda l, a=ql, b=kl, c=kl: ops.stem_tpd(l, a, b, c, 128, 1.0, 4, 4, 0.2, 30, 0.1, 30)  # noqa: E731
    bad += [
        lambda: tpd(lg.float()),
        lambda: tpd(torch.zeros(1, 2, 4, 3, device=dev, dtype=BF).transpose(2, 3)),
        lambda: tpd(lg, a=ql.long()),
        lambda: tpd(lg, b=kl.long()),
        lambda: tpd(lg, c=kl.long()),
        lambda: tpd(lg, c=i32(1, 2)),
        lambda: tpd(torch.zeros(1, 1, 1, 32769, device=dev, dtype=BF)),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail(f"case {i} was not refused")
