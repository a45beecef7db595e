"""Decode attention at GQA groups 1, 2 and 16 (num_head_q / num_head_kv; the prefill ops take 1 / 2 / 4 / 8 / 16 and so
does decode), on needle inputs against the pinned oracle with the scale-aware bar - the checks of
tests/test_attention_decode_needles.py, on the forms the new groups reach:

* head pairs (<= 16 q rows per kv head, NHD pages, even kv head count): 8 / 8 and 8 / 16 heads at every page size, one q
  token and the op's maximum; 4 / 64 heads at one q token;
* one kv head per workgroup (17 ... 32 rows): 4 / 64 and 2 / 32 heads at two q tokens, NHD and HND pages;
* first generation: 3 / 3, 1 / 16, 1 / 2 heads, HND pages with <= 16 rows;
* group 16 at num_seq_q >= 3, 48 ... 80 q rows per kv head: more than a form holds (bf16 48 rows: the first generation's
  three-block form) - the kv head's 16 q heads run as 2 slices of 8: virtual kv heads of the one-head form
  (csrc/attention_decode.hip::decode_slices), or one first-generation pass per slice (fp8 on pages of 16, bf16 num_seq_q 5);
* development keys (marked `dev`): the first generation forced (12 = 1 fp8, 28 = 1 bf16) and the one-head form for every
  eligible call (60 = 3) at groups 1, 2 and 16;
* groups 3 and 32 stay refused, by the C entry (HPC_ERR_UNSUPPORTED before any device call) and by the torch op.

Bars: decode_needles.TAU_NEEDLE_* unchanged.  They were calibrated at groups 4 / 8; test_split_model_within_tau_new_groups
checks on the CPU that the split-K model stays inside them at the new head ratios, sliced row counts included.  Every GPU
check compares the longest request of its case and runs the wrong-page negative control.

decode_needles.needle_inputs stops at 32 q rows per kv head; `needle_inputs` below is that generator with the bound
at 96 rows (a q row's needle coordinate is one of 0 ... num_seq_q * G - 1 of the 128; q carries its noise on the
coordinates past them, of which at least 32 remain)."""
import ctypes
import functools
import math
from pathlib import Path

import pytest
import torch

import decode_needles as dn
from test_attention_decode_needles import KTOK, PT, _call, _rows, _wrong_page
from utils import attn_close, attn_rel_err, dev_set

ROOT = Path(__file__).resolve().parents[1]
F8 = torch.float8_e4m3fn
D = dn.D
_KINDS = [("fp8", PT), ("fp8", KTOK), ("bf16", PT)]


def needle_inputs(lens_before, num_seq_q, P, heads, kind="fp8", k_per_token=False, seed=0, device="cpu", combs=True):
    """decode_needles.needle_inputs (same plan, same draws, same poison) for up to 96 q rows per kv head"""
    Hkv, Hq = heads
    G, Sq = Hq // Hkv, num_seq_q
    assert Sq * G <= 96 and Sq * G + 32 <= D
    lens_before = lens_before.to(torch.int32).cpu()
    lens_total = lens_before + Sq
    gen = torch.Generator().manual_seed(seed)
    block_ids, nblocks, pool, spare = dn._pages(lens_total, P, max(4, int(dn.nblocks_sum(lens_total, P)) // 16), gen)
    keys, alpha = dn._plan(lens_before, Sq, P, heads, gen, combs)
    dgen = torch.Generator(device=device).manual_seed(seed)
    K = torch.randn(pool, P, Hkv, D, generator=dgen, device=device) * dn.SIGMA_K
    V = torch.randn(pool, P, Hkv, D, generator=dgen, device=device)
    npos = Sq * G
    tails = [(int(block_ids[b, nb - 1]), int(lens_total[b]) - (nb - 1) * P) for b, nb in enumerate(nblocks.tolist())]
    for page, first in tails:
        if first < P:
            K[page, first:, :, :npos] = dn.POISON
            V[page, first:] *= 4
    if len(spare):
        sp = spare.long().to(device)
        K[sp, :, :, :npos] = dn.POISON
        V[sp] *= 4
    if keys:
        kt = torch.tensor([(int(block_ids[b, t // P]), t % P, g, j) for b, t, g, j, _ in keys], dtype=torch.long)
        vals = torch.tensor([v for *_, v in keys], dtype=torch.float32, device=device)
        kt = kt.to(device)
        K[kt[:, 0], kt[:, 1], kt[:, 2]] = 0
        K[kt[:, 0], kt[:, 1], kt[:, 2], kt[:, 3]] = vals
    q = torch.randn(len(lens_total) * Sq, Hq, D, generator=dgen, device=device) * dn.SIGMA_Q
    q[:, :, :npos] = 0
    own = torch.tensor([(r, h, (r % Sq) * G + h % G) for r in range(len(lens_total) * Sq) for h in range(Hq)],
                       dtype=torch.long, device=device)
    q[own[:, 0], own[:, 1], own[:, 2]] = (alpha.to(device) * math.sqrt(D)).reshape(-1)
    out = dict(block_ids=block_ids, nblocks=nblocks, lens_before=lens_before, lens_total=lens_total, spare=spare,
               num_seq_q=Sq, P=P, heads=heads, kind=kind, k_per_token=k_per_token)
    if kind == "bf16":
        out["q"] = q.to(torch.bfloat16)
        out["kv"] = torch.stack([K, V], 1).to(torch.bfloat16)
        return out
    q_scale = q.abs().amax(-1) / 448
    out["q"], out["q_scale"] = (q / q_scale[:, :, None]).to(F8), q_scale
    rows = P * 4 // D if k_per_token else 0
    kv = torch.zeros(pool, 2, P + rows, Hkv, D, dtype=F8, device=device)
    if k_per_token:
        from oracle import attention as oattn

        kfull = torch.zeros(pool, P + rows, Hkv, D, device=device)
        kfull[:, :P] = K
        kv[:, 0], _ = oattn.quant_paged_cache_pertoken(kfull, P)
        out["k_scale"] = kv[:, 0, P:]
        v_scale = V.abs().amax((0, 1, 3)) / 448
        kv[:, 1, :P] = (V / v_scale[None, None, :, None]).to(F8)
    else:
        k_scale = (K.abs().amax() / 448).reshape(1)
        v_scale = (V.abs().amax() / 448).reshape(1)
        kv[:, 0] = (K / k_scale).to(F8)
        kv[:, 1] = (V / v_scale).to(F8)
        out["k_scale"] = k_scale
    out["kv"], out["v_scale"] = kv, v_scale
    return out


def test_wide_generator_is_the_projects_generator():
    """the copy above draws exactly what decode_needles.needle_inputs draws wherever both are defined"""
    lens = torch.tensor([0, 1, 63, 700, 1500], dtype=torch.int32)
    for kind, quant in _KINDS:
        a = dn.needle_inputs(lens, 2, 32, (2, 32), kind, quant == KTOK, seed=11)
        b = needle_inputs(lens, 2, 32, (2, 32), kind, quant == KTOK, seed=11)
        for key in ("q", "kv", "block_ids", "q_scale", "k_scale", "v_scale"):
            if key in a:
                assert torch.equal(a[key].view(torch.uint8) if a[key].dtype == F8 else a[key],
                                   b[key].view(torch.uint8) if b[key].dtype == F8 else b[key]), (kind, quant, key)


# ---- CPU: the bars hold at the new head ratios ------------------------------------------------------------------------
_BAR_HEADS = [(8, 8), (8, 16), (4, 64), (2, 32), (1, 16), (3, 3)]
_SLICED = [((4, 64), 4), ((2, 32), 3), ((2, 32), 4), ((1, 16), 3)]   # (heads, num_seq_q) with 48 ... 64 q rows per kv head


@pytest.mark.parametrize("heads", _BAR_HEADS, ids=lambda h: f"{h[0]}-{h[1]}")
@pytest.mark.parametrize("kind,quant", _KINDS)
def test_split_model_within_tau_new_groups(kind, quant, heads):
    """tests/test_attn_bar.py::test_split_model_within_tau at the head ratios this file adds: the split-K model
    (decode_needles.split_model, every RANGE_LENS) against the oracle on the edge lengths, seed 11, num_seq_q 1 ... 4
    (bf16 4 / 64 heads: 5 too) - rows per kv head up to 80, the sliced calls included - stays within the project's bar; and
    on the sliced row counts the causal-mask mutant (row s sees one token too many) is off by more than 10 x the row's scale."""
    tau = dn.needle_tau(kind, quant == KTOK)
    worst = 0.0
    for Sq in range(1, 6 if (kind == "bf16" and heads == (4, 64)) else 5):
        inp = needle_inputs(dn.edge_lens(64, Sq), Sq, 64, heads, kind, quant == KTOK, seed=11)
        ref = dn.oracle(inp)
        w = max(float(attn_rel_err(ref, dn.split_model(inp, R), Sq).max()) for R in dn.RANGE_LENS)
        print(f"\nsplit model {kind} {quant} heads={heads[0]}/{heads[1]} Sq={Sq}: worst {w:.4f} (tau {tau})")
        worst = max(worst, w)
        if (heads, Sq) in _SLICED or Sq == 5:
            mut = float(attn_rel_err(ref, dn.split_model(inp, causal_shift=1), Sq).max())
            print(f"  causal_shift = 1 mutant: {mut:.3f} x the row scale")
            assert mut > 10, mut
    print(f"split model {kind} {quant} heads={heads[0]}/{heads[1]}: worst {worst:.4f} <= tau {tau}")
    assert worst <= tau, (worst, tau)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_cabi_refuses_groups_3_and_32():
    """the host check of both C entries answers HPC_ERR_UNSUPPORTED (-1) for a head ratio outside {1, 2, 4, 8, 16} before
    any device call (no GPU needed: the pointers are never dereferenced on the host)"""
    from ctypes import c_int, c_int64, c_void_p

    lib = ctypes.CDLL(str(ROOT / "hpc-ops_amd" / "hpc" / "libhpc_amd.so"))
    p = c_void_p(4096)
    bf16 = lib.hpc_attention_decode_bf16_async
    bf16.restype = c_int
    bf16.argtypes = [c_void_p] * 8 + [c_int] * 12 + [c_int64] * 6 + [c_void_p]
    fp8 = lib.hpc_attention_decode_fp8_async
    fp8.restype = c_int
    fp8.argtypes = [c_void_p] * 11 + [c_int] * 14 + [c_int64] * 9 + [c_void_p]
    for hq, hkv in [(3, 1), (12, 4), (32, 1), (64, 2), (6, 1), (5, 1)]:
        # new_kv_included, bins, B, Sq, Hq, Hkv, D, D, page, max blocks, ldY, ldQ
        ints = (1, 256, 2, 1, hq, hkv, 128, 128, 64, 4, hq * 128, hq * 128)
        strides = (64 * hkv * 128, hkv * 128, 128) * 2
        assert bf16(*([p] * 8), *ints, *strides, None) == -1, (hq, hkv)
        # new_kv_included, quant_type, bins, B, Sq, Hq, Hkv, D, D, page, max blocks, qscale stride, ldY, ldQ
        ints8 = (1, 1, 256, 2, 1, hq, hkv, 128, 128, 64, 4, hq, hq * 128, hq * 128)
        assert fp8(*([p] * 11), *ints8, *strides, 0, 0, 0, None) == -1, (hq, hkv)


@pytest.mark.gpu
@pytest.mark.parametrize("heads", [(1, 3), (2, 6), (1, 32), (1, 12)], ids=lambda h: f"{h[0]}-{h[1]}")
def test_torch_ops_refuse_other_groups(heads):
    import hpc

    Hkv, Hq = heads
    bid = torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    lens = torch.tensor([3, 4], dtype=torch.int32, device="cuda")
    q = torch.randn(2, Hq, 128, dtype=torch.bfloat16, device="cuda")
    kv = torch.randn(4, 64, Hkv, 128, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="1, 2, 4, 8 or 16"):
        hpc.attention_decode_bf16(q, kv, kv, bid, lens)
    one = torch.ones(1, device="cuda")
    with pytest.raises(RuntimeError, match="1, 2, 4, 8 or 16"):
        hpc.attention_decode_fp8(q.to(F8), kv.to(F8), kv.to(F8), bid, lens, torch.ones(2, Hq, device="cuda"), one, one)


# ---- GPU --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _case(name, heads, kind, quant, P, Sq, seed=11):
    """device inputs + the oracle on the compared rows (edges: all; named cases: the long requests and a sample)"""
    if name == "edges":
        lens_before = dn.edge_lens(P, Sq)
        rows = list(range(len(lens_before)))
    else:
        lens_before = (torch.tensor(dn.NAMED_CASES[name], dtype=torch.int32) - Sq).clamp_min(0)
        rows = _rows(lens_before + Sq)
    inp = needle_inputs(lens_before, Sq, P, heads, kind, quant == KTOK, seed=seed, device="cuda")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    assert int(torch.argmax(inp["lens_total"])) in rows  # the longest request is always compared
    return inp, rows, dn.oracle(inp, rows)


def _check(form, name, heads, kind, quant, P, Sq, layout="NHD", new_kv_included=True, use_task_map=True):
    """tests/test_attention_decode_needles.py::_check on this file's generator"""
    inp, rows, ref = _case(name, heads, kind, quant, P, Sq)
    tau = dn.needle_tau(kind, quant == KTOK)
    y = _call(inp, inp["block_ids"], layout, new_kv_included, use_task_map, rows)
    worst = float(attn_rel_err(ref, y, Sq).max())
    print(f"NEEDLE {form} {kind} {quant} {name} heads={heads[0]}/{heads[1]} P={P} Sq={Sq} {layout} "
          f"new_kv={int(new_kv_included)} tm={int(use_task_map)}: worst {worst:.4f} (tau {tau})")
    assert attn_close(ref, y, tau, Sq, label=f"{form} {name}")
    y_bad = _call(inp, _wrong_page(inp), layout, new_kv_included, use_task_map, rows)
    assert not attn_close(ref, y_bad, tau, Sq, label="negative control (expected to fail)")


_SETTINGS = [(True, True), (False, True), (True, False)]  # (new_kv_included, task map) of test_needles_fp8_head_pair_edges


def _max_sq(kind):
    return 5 if kind == "bf16" else 4


# (the op takes per-token K scales on pages of 32 / 64 only: a scale row holds 32 tokens)
_PAIR_EDGES = [(kind, quant, P) for kind, quant in _KINDS for P in (16, 32, 64) if not (quant == KTOK and P == 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("sq_max", [False, True], ids=["sq1", "sqmax"])
@pytest.mark.parametrize("kind,quant,P", _PAIR_EDGES)
@pytest.mark.parametrize("heads", [(8, 8), (8, 16)], ids=lambda h: f"{h[0]}-{h[1]}")
def test_groups_1_2_head_pair_edges(heads, kind, quant, P, sq_max):
    """groups 1 and 2 on the head-pair kernels: 1 ... 10 q rows per kv head, pages of 16 / 32 / 64, edge lengths, with and
    without new_kv_included and a task map"""
    Sq = _max_sq(kind) if sq_max else 1
    for new_kv_included, use_task_map in _SETTINGS:
        _check("pair", "edges", heads, kind, quant, P, Sq, "NHD", new_kv_included, use_task_map)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,quant", _KINDS)
@pytest.mark.parametrize("name", ["one_128k_31x4k", "edges"])
def test_group_16_head_pair(name, kind, quant):
    """group 16, one q token = 16 rows per kv head: the head-pair kernels with full tiles"""
    _check("pair", name, (4, 64), kind, quant, 64, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,quant", _KINDS)
@pytest.mark.parametrize("name", ["one_64k_31x4k", "edges"])
@pytest.mark.parametrize("heads", [(4, 64), (2, 32)], ids=lambda h: f"{h[0]}-{h[1]}")
def test_group_16_solo(heads, name, kind, quant):
    """group 16, two q tokens = 32 rows per kv head: one kv head per workgroup, NHD and HND pages"""
    for layout in ("NHD", "HND"):
        _check("solo", name, heads, kind, quant, 64 if name != "edges" else 32, 2, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("name,heads,Sq,P,layout,kind,quant", [
    ("edges", (3, 3), 4, 64, "NHD", "fp8", PT),
    ("edges", (3, 3), 5, 16, "NHD", "bf16", PT),
    ("skewed_extreme", (3, 3), 1, 32, "HND", "fp8", KTOK),
    ("skewed_extreme", (1, 16), 1, 64, "NHD", "fp8", KTOK),
    ("edges", (1, 16), 1, 16, "NHD", "fp8", PT),
    ("edges", (1, 16), 2, 16, "NHD", "fp8", PT),          # 32 rows on pages of 16: the two-block form
    ("edges", (1, 2), 4, 64, "NHD", "fp8", PT),
    ("edges", (1, 2), 5, 32, "HND", "bf16", PT),
    ("two_32k_30x4k", (8, 8), 2, 64, "HND", "fp8", PT),
    ("edges", (8, 16), 4, 32, "HND", "fp8", KTOK),
    ("edges", (4, 64), 1, 64, "HND", "bf16", PT),
])
def test_new_groups_first_generation(name, heads, Sq, P, layout, kind, quant):
    """odd kv head counts (3 / 3, 1 / 16, 1 / 2 heads) and HND pages with <= 16 rows: the first-generation kernel from the task map"""
    _check("first_gen", name, heads, kind, quant, P, Sq, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,quant,Sq", [("fp8", PT, 3), ("fp8", PT, 4), ("fp8", KTOK, 3), ("fp8", KTOK, 4),
                                           ("bf16", PT, 3), ("bf16", PT, 4), ("bf16", PT, 5)])
@pytest.mark.parametrize("heads", [(4, 64), (1, 16)], ids=lambda h: f"{h[0]}-{h[1]}")
def test_group_16_sliced_edges(heads, kind, quant, Sq):
    """group 16 at num_seq_q >= 3: 48 ... 80 q rows per kv head, served as 2 slices of 8 q heads per kv head - virtual kv heads of
    the one-head form, at bf16 num_seq_q 5 two passes of the three-block form (bf16 num_seq_q 3: one pass of that form)"""
    for layout, P in (("NHD", 32), ("HND", 64)):
        if layout == "HND":
            _check("sliced", "edges", heads, kind, quant, P, Sq, layout, new_kv_included=False, use_task_map=False)
        else:
            _check("sliced", "edges", heads, kind, quant, P, Sq, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("name,heads,Sq,P,layout,kind,quant", [
    ("one_64k_31x4k", (4, 64), 4, 64, "NHD", "fp8", PT),
    ("two_32k_30x4k", (4, 64), 3, 32, "HND", "fp8", KTOK),
    ("one_128k_31x4k", (1, 16), 5, 64, "HND", "bf16", PT),
    ("one_64k_31x4k", (4, 64), 3, 16, "NHD", "bf16", PT),
])
def test_group_16_sliced_named(name, heads, Sq, P, layout, kind, quant):
    """sliced calls on the long named cases: requests split over many ranges, merged per slice"""
    _check("sliced", name, heads, kind, quant, P, Sq, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("heads,Sq", [((4, 64), 3), ((1, 16), 4)])
def test_group_16_sliced_pages_of_16_fp8(heads, Sq):
    """fp8 on pages of 16 has no one-head form: the sliced call runs as one first-generation pass per slice of 8 q heads"""
    _check("sliced_first_gen", "edges", heads, "fp8", PT, 16, Sq)


_DEV_FORMS = [  # (key, value, name, heads, Sq, P, layout, kind, quant)
    (12, 1, "edges", (8, 8), 4, 64, "NHD", "fp8", PT),            # first generation forced, fp8: groups 1, 2, 16
    (12, 1, "edges", (8, 16), 1, 32, "NHD", "fp8", KTOK),
    (12, 1, "one_64k_31x4k", (4, 64), 1, 64, "NHD", "fp8", PT),
    (12, 1, "edges", (4, 64), 2, 64, "NHD", "fp8", KTOK),
    (28, 1, "edges", (8, 8), 5, 16, "NHD", "bf16", PT),           # ... bf16
    (28, 1, "edges", (8, 16), 1, 64, "NHD", "bf16", PT),
    (28, 1, "edges", (4, 64), 2, 64, "NHD", "bf16", PT),          # 32 rows: the two-block form instead of one head per workgroup
    (12, 1, "edges", (4, 64), 4, 32, "HND", "fp8", KTOK),         # sliced: one first-generation pass per slice
    (12, 1, "two_32k_30x4k", (2, 32), 3, 64, "NHD", "fp8", PT),
    (28, 1, "edges", (4, 64), 5, 64, "NHD", "bf16", PT),          # ... bf16: two passes of 40 rows on the three-block form
    (28, 1, "edges", (1, 16), 4, 16, "HND", "bf16", PT),
    (60, 3, "edges", (8, 8), 4, 32, "NHD", "fp8", PT),            # one kv head per workgroup for every eligible call
    (60, 3, "edges", (8, 16), 1, 64, "HND", "fp8", KTOK),
    (60, 3, "one_64k_31x4k", (4, 64), 1, 64, "NHD", "fp8", PT),
    (60, 3, "edges", (2, 4), 5, 16, "NHD", "bf16", PT),
]


@pytest.mark.dev
@pytest.mark.gpu
@pytest.mark.parametrize("key,value,name,heads,Sq,P,layout,kind,quant", _DEV_FORMS)
def test_new_groups_dev_forms(key, value, name, heads, Sq, P, layout, kind, quant):
    dev_set(key, value)
    try:
        _check(f"dev{key}={value}", name, heads, kind, quant, P, Sq, layout)
    finally:
        dev_set(key, 0)
