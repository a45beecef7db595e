"""Decode attention on needle inputs (tests/decode_needles.py) against the pinned oracles, with the scale-aware bar
tests/utils.py::attn_close, on every dispatch form - reached the way the other decode tests reach them:

* fp8 head-pair kernel (even kv head count, <= 16 q rows per kv head, NHD pages): the product path, pages of 16 / 32 / 64,
  per-tensor and per-token K scales;
* fp8 kSolo (17 ... 32 q rows per kv head), NHD and HND pages, both quant types;
* fp8 first generation (one / odd kv heads, HND pages with <= 16 q rows);
* development forms (marked `dev`, re-run by tests/test_dev_build.py): four heads per workgroup (key 29 = 2), the first
  generation forced (key 12 = 1), kSolo everywhere (key 60 = 3), the combine-kernel merge (key 33 = 1);
* bf16 head-pair, one-head (17 ... 32 rows) and first-generation (key 28 = 1) forms.

Lengths: the reference benchmark's named cases (decode_needles.NAMED_CASES, up to one 128k-token request split across the
whole grid) at 1 / 8 and 8 / 64 heads, and edge lengths (empty caches, 1 token, = 0, 1, P - 1 mod P) with and without
new_kv_included and a task map.  The long requests are always compared, the others sampled.  Every test also runs a
negative control on real kernel output: the same call with a wrong page in the longest request's block table
must FAIL attn_close against the oracle - the bar has teeth on the device, not only in the CPU mutation test
(tests/test_attn_bar.py).  The worst error of each call is printed (`NEEDLE ...` lines; pytest -rP)."""
import functools

import pytest
import torch

import decode_needles as dn
from utils import attn_close, attn_rel_err, dev_set

F8 = torch.float8_e4m3fn
PT, KTOK = "per_tensor", "per_token_k"


def _rows(lens_total, every=None):
    """the long requests (>= 16k tokens, the longest among them) and a sample of the others"""
    n = len(lens_total)
    long = [i for i in range(n) if int(lens_total[i]) >= 16384] + [int(torch.argmax(lens_total))]
    step = every or max(1, n // 6)
    return sorted(set(long) | set(range(0, n, step)) | {n - 1})


@functools.lru_cache(maxsize=2)
def _case(name, heads, kind, quant, P, Sq, seed=11):
    """device inputs + the oracle on the sampled rows; built once per (case, heads, ...) in a worker (the 128k cases)"""
    if name == "edges":
        lens_before = dn.edge_lens(P, Sq)
        rows = list(range(len(lens_before)))
    else:
        lens_before = (torch.tensor(dn.NAMED_CASES[name], dtype=torch.int32) - Sq).clamp_min(0)
        rows = _rows(lens_before + Sq)
    inp = dn.needle_inputs(lens_before, Sq, P, heads, kind, quant == KTOK, seed=seed, device="cuda")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    return inp, rows, dn.oracle(inp, rows)


def _wrong_page(inp):
    """the block table with the longest request's last page replaced by a pool page outside every table (poisoned).
    (Two full pages of one request swapped would not do: attention is invariant under a permutation of the keys, so
    the right answer does not change unless the page holds a partial tail or the speculative rows' causal edge.)"""
    b = int(torch.argmax(inp["lens_total"]))
    bad = inp["block_ids"].clone()
    bad[b, int(inp["nblocks"][b]) - 1] = inp["spare"][0]
    return bad


def _call(inp, block_ids, layout, new_kv_included, use_task_map, out_rows):
    import hpc

    P, Sq = inp["P"], inp["num_seq_q"]
    Hkv, Hq = inp["heads"]
    kv = inp["kv"]
    if layout == "HND":
        kv = kv.view(torch.uint8).permute(0, 1, 3, 2, 4).contiguous().permute(0, 1, 3, 2, 4).view(kv.dtype)
    lens_in = (inp["lens_total"] if new_kv_included else inp["lens_before"]).cuda()
    tm = None
    if use_task_map:
        tm = hpc.get_attention_decode_task_workspace(len(lens_in), int(inp["lens_total"].max()), Hkv, min_process_len=64)
        hpc.assign_attention_decode_task(lens_in, tm, Hkv, Sq, new_kv_included, min_process_len=64)
    bd = block_ids.cuda()
    if inp["kind"] == "bf16":
        y = hpc.attention_decode_bf16(inp["q"], kv[:, 0], kv[:, 1], bd, lens_in, mtp=Sq - 1, new_kv_included=new_kv_included,
                                      splitk=True, task_map=tm)
    else:
        ktok = inp["k_per_token"]
        qt = (hpc.QuantType.QPERTOKEN_PERHEAD_KPERTOKEN_PERHEAD_VPERHEAD if ktok
              else hpc.QuantType.QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR)
        ks = kv[:, 0, P:] if ktok else inp["k_scale"]
        y = hpc.attention_decode_fp8(inp["q"], kv[:, 0, :P], kv[:, 1, :P], bd, lens_in, inp["q_scale"], ks, inp["v_scale"],
                                     mtp=Sq - 1, new_kv_included=new_kv_included, quant_type=qt, splitk=True, task_map=tm)
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16
    return y.reshape(-1, Sq, Hq, y.shape[-1])[out_rows].cpu()


def _check(form, name, heads, kind, quant, P, Sq, layout="NHD", new_kv_included=True, use_task_map=True):
    inp, rows, ref = _case(name, heads, kind, quant, P, Sq)
    tau = dn.needle_tau(kind, quant == KTOK)
    y = _call(inp, inp["block_ids"], layout, new_kv_included, use_task_map, rows)
    worst = float(attn_rel_err(ref, y, Sq).max())
    print(f"NEEDLE {form} {kind} {quant} {name} heads={heads[0]}/{heads[1]} P={P} Sq={Sq} {layout} "
          f"new_kv={int(new_kv_included)} tm={int(use_task_map)}: worst {worst:.4f} (tau {tau})")
    assert attn_close(ref, y, tau, Sq, label=f"{form} {name}")
    # negative control: a wrong page in the longest request's table -> the bar must fail
    y_bad = _call(inp, _wrong_page(inp), layout, new_kv_included, use_task_map, rows)
    assert not attn_close(ref, y_bad, tau, Sq, label="negative control (expected to fail)")


_HEADS = [(1, 8), (8, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("quant", [PT, KTOK])
@pytest.mark.parametrize("heads", _HEADS)
@pytest.mark.parametrize("name", list(dn.NAMED_CASES))
def test_needles_fp8_named_cases(name, heads, quant):
    """one q row: 8 / 64 heads = the head-pair kernel, 1 / 8 heads (one kv head) = the first generation"""
    _check("pair" if heads[0] % 2 == 0 else "first_gen", name, heads, "fp8", quant, 64, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("new_kv_included,use_task_map", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("P,quant", [(16, PT), (32, PT), (64, PT), (32, KTOK), (64, KTOK)])
def test_needles_fp8_head_pair_edges(P, quant, new_kv_included, use_task_map):
    """16 q rows per kv head (Sq 2 at group 8) on the head-pair kernel: edge lengths, pages of 16 / 32 / 64"""
    _check("pair", "edges", (8, 64), "fp8", quant, P, 2, "NHD", new_kv_included, use_task_map)


@pytest.mark.gpu
@pytest.mark.parametrize("quant", [PT, KTOK])
@pytest.mark.parametrize("layout", ["NHD", "HND"])
@pytest.mark.parametrize("name,heads,Sq", [("one_64k_31x4k", (8, 64), 3), ("one_128k_31x4k", (1, 8), 4), ("edges", (4, 32), 4)])
def test_needles_fp8_solo(name, heads, Sq, layout, quant):
    """17 ... 32 q rows per kv head: one kv head per workgroup (kSolo)"""
    _check("solo", name, heads, "fp8", quant, 64, Sq, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("name,heads,Sq,layout,quant", [("two_32k_30x4k", (4, 32), 2, "HND", PT), ("edges", (4, 32), 2, "HND", KTOK),
                                                        ("skewed_extreme", (3, 24), 1, "NHD", PT), ("edges", (1, 8), 2, "NHD", PT)])
def test_needles_fp8_first_generation(name, heads, Sq, layout, quant):
    """HND pages with <= 16 q rows, odd kv head counts: the first-generation kernel"""
    _check("first_gen", name, heads, "fp8", quant, 64, Sq, layout)


_DEV_FORMS = [  # (key, value, name, heads, Sq, P, layout, quant)
    (29, 2, "two_32k_30x4k", (8, 64), 1, 64, "NHD", PT),      # four heads per workgroup
    (29, 2, "edges", (8, 64), 1, 16, "NHD", PT),
    (12, 1, "one_128k_31x4k", (8, 64), 1, 64, "NHD", PT),     # first generation forced
    (12, 1, "edges", (8, 64), 2, 64, "NHD", KTOK),
    (60, 3, "one_64k_31x4k", (8, 64), 1, 64, "NHD", PT),      # kSolo for every eligible call
    (60, 3, "edges", (2, 16), 1, 32, "HND", KTOK),
    (33, 1, "one_64k_31x4k", (1, 8), 1, 64, "NHD", PT),       # first generation, combine-kernel merge
    (33, 1, "edges", (4, 32), 2, 64, "HND", KTOK),
]


@pytest.mark.dev
@pytest.mark.gpu
@pytest.mark.parametrize("key,value,name,heads,Sq,P,layout,quant", _DEV_FORMS)
def test_needles_fp8_dev_forms(key, value, name, heads, Sq, P, layout, quant):
    dev_set(key, value)
    try:
        _check(f"dev{key}={value}", name, heads, "fp8", quant, P, Sq, layout)
    finally:
        dev_set(key, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("heads", _HEADS)
@pytest.mark.parametrize("name", list(dn.NAMED_CASES))
def test_needles_bf16_named_cases(name, heads):
    """bf16, one q row: 8 / 64 heads = the head-pair kernel, 1 / 8 heads = the first generation"""
    _check("pair" if heads[0] % 2 == 0 else "first_gen", name, heads, "bf16", PT, 64, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,heads,Sq,P,layout,new_kv_included", [("edges", (8, 64), 2, 16, "NHD", False),
                                                                    ("edges", (8, 64), 2, 32, "NHD", True),
                                                                    ("one_64k_31x4k", (8, 64), 3, 64, "NHD", True),
                                                                    ("edges", (4, 32), 4, 32, "HND", False)])
def test_needles_bf16_forms(name, heads, Sq, P, layout, new_kv_included):
    """bf16 head pairs with 16 rows (pages of 16 / 32) and the one-head form (24 / 32 rows)"""
    _check("pair" if Sq * heads[1] // heads[0] <= 16 else "solo", name, heads, "bf16", PT, P, Sq, layout, new_kv_included)


@pytest.mark.dev
@pytest.mark.gpu
@pytest.mark.parametrize("name,heads,Sq", [("one_128k_31x4k", (1, 8), 1), ("two_32k_30x4k", (8, 64), 1), ("edges", (8, 64), 2)])
def test_needles_bf16_first_generation(name, heads, Sq):
    """development key 28 = 1: bf16 on the first-generation kernel"""
    dev_set(28, 1)
    try:
        _check("dev28=1", name, heads, "bf16", PT, 64, Sq)
    finally:
        dev_set(28, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["base", "block_stride"])
def test_per_token_k_scale_misaligned_view_is_rejected(what):
    """the kernels load per-token K scales as dwords: a scale view whose base or page stride is not a multiple of 4 bytes
    is refused by the op before any launch"""
    import hpc

    inp = dn.needle_inputs(torch.tensor([100, 3], dtype=torch.int32), 1, 64, (2, 16), "fp8", True, device="cuda")
    kv, P = inp["kv"], 64
    ks = kv[:, 0, P:]
    if what == "base":
        bad = ks.as_strided(ks.shape, ks.stride(), ks.storage_offset() + 1)
    else:
        s = ks.stride()
        buf = torch.zeros(ks.shape[0] * (s[0] + 1) + 16, dtype=F8, device="cuda")
        bad = buf.as_strided(ks.shape, (s[0] + 1, s[1], s[2], s[3]))
    with pytest.raises(RuntimeError, match="multiples of 4 bytes"):
        hpc.attention_decode_fp8(inp["q"], kv[:, 0, :P], kv[:, 1, :P], inp["block_ids"].cuda(), inp["lens_total"].cuda(),
                                 inp["q_scale"], bad, inp["v_scale"], mtp=0, new_kv_included=True,
                                 quant_type=hpc.QuantType.QPERTOKEN_PERHEAD_KPERTOKEN_PERHEAD_VPERHEAD, splitk=True)
