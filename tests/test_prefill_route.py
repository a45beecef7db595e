"""Which prefill-attention kernel form a call runs, with which shifts and on which grid, or why it is refused:
csrc/attention_prefill_route.h::prefill_route(), a pure host function, asked through the development build's hpc_dev_prefill_route
(flat arrays: the members of PrefillCall in, those of PrefillRoute out).  No GPU.  The rows are the table of DESIGN 3.9."""
import ctypes
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
OK, UNSUPPORTED, INVALID = 0, -1, -2
FP8, FP8_SPARSE, BF16_PAGED, BF16 = 0, 1, 2, 3  # PrefillEntry
ROUTE = ("code", "empty", "g_shift", "page_shift", "quant", "sparse", "by_head", "v_perm", "grid_x", "grid_y", "grid_z", "threads")
KEYS = (7, 46)  # every key prefill_route() reads


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(str(ROOT / "hpc-ops_amd" / "hpc" / "libhpc_amd_dev.so"))
    lib.hpc_dev_prefill_route.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    return lib


def call(entry=FP8, qt=1, mask=None, batch=4, sq=256, dims=(128, 128), kv=8, group=8, page=64, **over):
    """PrefillCall of a cache in the usual NHD layout [page][token][head][128], strides in elements; quant_type 0 keeps four tail
    rows of K scales per page.  mask = (mask_tiles_m, mask_tiles_kv).  Contiguous bf16: no pages, rows kv * 128 apart.
    `over` replaces members by name after the layout is made (hkv, ldQ, ldY, kb, kt, kh, vb, vt, vh)."""
    token, head = 128 * kv, 128
    block = token * (page + (4 if entry in (FP8, FP8_SPARSE) and qt == 0 else 0))
    if entry == BF16:
        page, block = 0, 0
    m = dict(hkv=kv, ldQ=128 * kv * group, ldY=128 * kv * group, kb=block, kt=token, kh=head, vb=block, vt=token, vh=head)
    assert set(over) <= set(m), over
    m.update(over)
    tm, tkv = mask or (0, 0)
    return [entry, qt, int(mask is not None), tm, tkv, batch, sq, dims[0], dims[1], kv * group, m["hkv"], page, m["ldQ"], m["ldY"],
            m["kb"], m["kt"], m["kh"], m["vb"], m["vt"], m["vh"]]


def route(lib, c):
    cin = (ctypes.c_int64 * len(c))(*c)
    out = (ctypes.c_int * len(ROUTE))()
    assert lib.hpc_dev_prefill_route(cin, len(c), out, len(ROUTE)) == OK
    return dict(zip(ROUTE, out))


def runs(**more):
    return dict(code=OK, empty=0, threads=256, **more)


SPARSE = dict(entry=FP8_SPARSE, mask=(2, 8))
U, I = dict(code=UNSUPPORTED), dict(code=INVALID)
G32, G31 = 1 << 32, 1 << 31

# all keys 0: what the product runs
ROWS = [
    # every group, page size, quant type, dense and masked; the grid is (q row tiles, kv heads, requests)
    ("fp8_group1", dict(group=1), runs(g_shift=0, page_shift=6, quant=1, sparse=0, by_head=0, v_perm=0, grid_x=2, grid_y=8, grid_z=4)),
    ("fp8_group2_page32", dict(group=2, page=32), runs(g_shift=1, page_shift=5, grid_x=4)),
    ("fp8_group4_page16", dict(group=4, page=16), runs(g_shift=2, page_shift=4, grid_x=8)),
    ("fp8_group8", dict(group=8, kv=2, batch=3), runs(g_shift=3, grid_x=16, grid_y=2, grid_z=3)),
    ("fp8_group16", dict(group=16), runs(g_shift=4, grid_x=32, by_head=0)),
    ("fp8_qt0_page32", dict(qt=0, page=32), runs(quant=0, page_shift=5, sparse=0)),
    ("fp8_qt0_page64", dict(qt=0), runs(quant=0, page_shift=6)),
    ("sparse_group1", dict(**SPARSE, group=1), runs(g_shift=0, sparse=1, by_head=1, quant=1)),
    ("sparse_group2", dict(**SPARSE, group=2), runs(g_shift=1, sparse=1, by_head=1)),
    ("sparse_group4_page16", dict(**SPARSE, group=4, page=16), runs(g_shift=2, page_shift=4, sparse=1, by_head=1)),
    ("sparse_group8_qt0_page32", dict(**SPARSE, qt=0, page=32), runs(g_shift=3, page_shift=5, quant=0, sparse=1, by_head=1)),
    ("sparse_group16", dict(**SPARSE, group=16), runs(g_shift=4, sparse=1, by_head=0)),  # no head-major form at group 16
    ("sparse_entry_without_mask", dict(entry=FP8_SPARSE), runs(sparse=0, by_head=0)),  # dense
    ("sparse_mask_512_columns", dict(entry=FP8_SPARSE, mask=(2, 512)), runs(sparse=1)),
    ("bf16_paged_group1_page16", dict(entry=BF16_PAGED, group=1, page=16), runs(g_shift=0, page_shift=4, by_head=0, v_perm=0, grid_x=2)),
    ("bf16_paged_group2_page32", dict(entry=BF16_PAGED, group=2, page=32), runs(g_shift=1, page_shift=5)),
    ("bf16_paged_group4", dict(entry=BF16_PAGED, group=4), runs(g_shift=2, page_shift=6)),
    ("bf16_paged_group8", dict(entry=BF16_PAGED), runs(g_shift=3, grid_x=16, grid_y=8, grid_z=4)),
    ("bf16_paged_group16", dict(entry=BF16_PAGED, group=16), runs(g_shift=4, grid_x=32)),
    ("bf16_contiguous_group1", dict(entry=BF16, group=1), runs(g_shift=0, page_shift=6, grid_x=2)),
    ("bf16_contiguous_group8", dict(entry=BF16), runs(g_shift=3, page_shift=6, sparse=0, by_head=0, v_perm=0, grid_x=16, grid_y=8, grid_z=4)),
    ("bf16_contiguous_group16", dict(entry=BF16, group=16), runs(g_shift=4, grid_x=32)),
    # grid_x = ceil(max_seqlens_q * group / 128)
    ("rows_1", dict(group=1, sq=1), runs(grid_x=1)),
    ("rows_128", dict(group=8, sq=16), runs(grid_x=1)),
    ("rows_128_group16", dict(group=16, sq=8), runs(grid_x=1)),
    ("rows_129", dict(group=1, sq=129), runs(grid_x=2)),
    ("rows_132_bf16", dict(entry=BF16_PAGED, group=4, sq=33), runs(grid_x=2)),
    ("rows_128_bf16_contiguous", dict(entry=BF16, group=2, sq=64), runs(grid_x=1)),
    ("grid_y_z_at_the_limit", dict(kv=65535, group=1, batch=65535), runs(grid_y=65535, grid_z=65535)),
    # empty calls and refusals, alone and in pairs where the order shows
    ("no_request", dict(batch=0), dict(code=OK, empty=1)),
    ("no_q_token", dict(entry=BF16, sq=0), dict(code=OK, empty=1)),
    ("no_request_head_dim_64", dict(batch=0, dims=(64, 128)), dict(code=OK, empty=1)),  # empty comes before the head dims
    ("quant_type_2_no_request", dict(qt=2, batch=0), I),  # and the quant type before empty
    ("negative_batch", dict(batch=-1), I),
    ("negative_seq_bf16", dict(entry=BF16_PAGED, sq=-1), I),
    ("head_dim_64", dict(dims=(64, 128)), U),
    ("head_dim_v_64_bf16", dict(entry=BF16, dims=(128, 64)), U),
    ("page_8_no_kv_heads", dict(page=8, hkv=0), U),  # the page before the heads
    ("page_128_bf16", dict(entry=BF16_PAGED, page=128), U),
    ("qt0_page16", dict(qt=0, page=16), U),
    ("no_kv_heads", dict(hkv=0), I),
    ("heads_do_not_divide", dict(hkv=3), I),
    ("group_3", dict(kv=8, group=3), U),
    ("group_32_bf16", dict(entry=BF16, kv=1, group=32), U),
    ("mask_no_columns_ldq_8", dict(entry=FP8_SPARSE, mask=(2, 0), ldQ=8192 + 8), U),  # alignment before the mask's tile counts
    ("mask_no_columns_k_block_4g", dict(entry=FP8_SPARSE, mask=(2, 0), kb=G32), I),  # the tile counts before the stride limits
    ("mask_no_rows", dict(entry=FP8_SPARSE, mask=(0, 8)), I),
    ("mask_513_columns", dict(entry=FP8_SPARSE, mask=(2, 513)), U),
    # the block-sparse entry wants a page that divides a 128-token mask tile, before anything else
    ("sparse_page_48", dict(**SPARSE, page=48), U),
    ("sparse_page_48_quant_type_2", dict(**SPARSE, page=48, qt=2), U),
    ("sparse_page_48_no_request", dict(**SPARSE, page=48, batch=0), U),
    ("sparse_page_128", dict(**SPARSE, page=128), U),  # divides, but no kernel form
    ("sparse_page_0", dict(**SPARSE, page=0), U),  # was an integer division by zero
    ("sparse_page_0_quant_type_2", dict(**SPARSE, page=0, qt=2), U),
    ("sparse_page_negative", dict(**SPARSE, page=-16), U),
    ("dense_page_0_quant_type_2", dict(page=0, qt=2), I),  # the dense entry has no such first check
    # stride limits: fp8 block stride and token stride x page below 2^32 bytes, bf16 below 2^31 elements; zero and below refused
    ("no_kv_heads_k_block_4g_fp8", dict(hkv=0, kb=G32), I),  # fp8: the heads before the stride limits
    ("no_kv_heads_k_block_2g_bf16", dict(entry=BF16_PAGED, hkv=0, kb=G31), U),  # paged bf16: the stride limits before the heads
    ("bf16_k_block_below_2g", dict(entry=BF16_PAGED, kb=G31 - 8), runs()),
    ("bf16_k_block_2g", dict(entry=BF16_PAGED, kb=G31), U),
    ("bf16_v_block_2g", dict(entry=BF16_PAGED, vb=G31), U),
    ("bf16_v_token_x_page_2g", dict(entry=BF16_PAGED, vt=G31 // 64), U),
    ("bf16_v_token_x_page_below_2g", dict(entry=BF16_PAGED, page=32, vt=G31 // 64), runs()),
    ("fp8_k_block_below_4g", dict(kb=G32 - 16), runs()),
    ("fp8_k_block_4g", dict(kb=G32), U),
    ("fp8_v_block_below_4g", dict(vb=G32 - 8), runs()),
    ("fp8_v_block_4g", dict(vb=G32), U),
    ("fp8_k_token_x_page_4g", dict(kt=G32 // 64), U),
    ("fp8_k_token_x_page_below_4g", dict(kt=G32 // 64 - 16), runs()),
    ("fp8_k_block_2g_is_fine", dict(kb=G31), runs()),
    ("fp8_zero_v_token_stride", dict(vt=0), U),
    ("bf16_negative_k_block", dict(entry=BF16_PAGED, kb=-1024), U),
    ("bf16_contiguous_has_no_stride_limit", dict(entry=BF16, kt=0), runs()),  # ldK 0: every key row is row 0, as ever
    ("grid_y_above_65535", dict(kv=65536, group=1), U),
    ("grid_z_above_65535", dict(batch=65536), U),
    ("grid_z_above_65535_bf16", dict(entry=BF16, batch=65536), U),
    # Alignment, as the entries always had it - NOT symmetric for fp8 and not to be "fixed" here: ldQ and the K strides to 16
    # elements, ldY and the V strides to 8; bf16: everything to 8.
    ("fp8_ldq_8", dict(ldQ=8192 + 8), U),
    ("fp8_ldy_8", dict(ldY=8192 + 8), runs()),
    ("fp8_ldy_4", dict(ldY=8192 + 4), U),
    ("fp8_k_token_8", dict(kt=1024 + 8), U),
    ("fp8_v_token_8", dict(vt=1024 + 8), runs()),
    ("fp8_v_token_4", dict(vt=1024 + 4), U),
    ("fp8_k_head_8", dict(kh=128 + 8), U),
    ("fp8_v_head_8", dict(vh=128 + 8), runs()),
    ("fp8_v_head_4", dict(vh=128 + 4), U),
    ("fp8_k_block_8", dict(kb=65536 + 8), U),
    ("fp8_v_block_8", dict(vb=65536 + 8), runs()),
    ("fp8_v_block_4", dict(vb=65536 + 4), U),
    ("bf16_ldq_8", dict(entry=BF16_PAGED, ldQ=8192 + 8), runs()),
    ("bf16_ldq_4", dict(entry=BF16_PAGED, ldQ=8192 + 4), U),
    ("bf16_k_token_8", dict(entry=BF16_PAGED, kt=1024 + 8), runs()),
    ("bf16_k_token_4", dict(entry=BF16_PAGED, kt=1024 + 4), U),
    ("bf16_contiguous_ldk_4", dict(entry=BF16, kt=1024 + 4), U),
    ("bf16_contiguous_ldv_8", dict(entry=BF16, vt=1024 + 8), runs()),
]

# {development key: value}, then the call
KEY_ROWS = [
    ("key7_by_head_dense", {7: 1}, dict(), runs(sparse=0, by_head=1)),
    ("key7_by_position_sparse", {7: 2}, dict(**SPARSE), runs(sparse=1, by_head=0)),
    ("key7_by_head_group16", {7: 1}, dict(**SPARSE, group=16), runs(by_head=0)),
    ("key7_not_bf16", {7: 1}, dict(entry=BF16_PAGED), runs(by_head=0)),
    ("key46_v_perm_paged", {46: 1}, dict(entry=BF16_PAGED), runs(v_perm=1)),
    ("key46_v_perm_contiguous", {46: 1}, dict(entry=BF16), runs(v_perm=1)),
    ("key46_other_value", {46: 2}, dict(entry=BF16_PAGED), runs(v_perm=0)),
    ("key46_not_fp8", {46: 1}, dict(), runs(v_perm=0)),
]


def check(got, want):
    assert {k: got[k] for k in want} == want, got


@pytest.mark.parametrize("name,kw,want", ROWS, ids=[r[0] for r in ROWS])
def test_prefill_route(lib, name, kw, want):
    got = route(lib, call(**kw))
    check(got, want)
    if got["code"] != OK or got["empty"]:  # a refusal or an empty call sets nothing else
        assert not any(v for k, v in got.items() if k not in ("code", "empty")), got


@pytest.mark.parametrize("name,keys,kw,want", KEY_ROWS, ids=[r[0] for r in KEY_ROWS])
def test_prefill_route_development_key(lib, name, keys, kw, want):
    for key, value in keys.items():
        assert lib.hpc_dev_tuning_set(key, value) == 0
    try:
        check(route(lib, call(**kw)), want)
    finally:
        for key in keys:
            assert lib.hpc_dev_tuning_set(key, 0) == 0
    assert [lib.hpc_dev_tuning_get(key) for key in KEYS] == [0] * len(KEYS)


def test_marshalling_is_checked(lib):
    c = call()
    cin = (ctypes.c_int64 * len(c))(*c)
    out = (ctypes.c_int * len(ROUTE))()
    assert lib.hpc_dev_prefill_route(cin, len(c) - 1, out, len(ROUTE)) == INVALID
    assert lib.hpc_dev_prefill_route(cin, len(c), out, len(ROUTE) - 1) == INVALID
    assert lib.hpc_dev_prefill_route(None, len(c), out, len(ROUTE)) == INVALID
    assert lib.hpc_dev_prefill_route(cin, len(c), None, len(ROUTE)) == INVALID


def test_keys_are_zero_after_the_key_rows(lib):
    """every key row puts its keys back (a key left set would re-route the GPU tests of the same process)"""
    assert [lib.hpc_dev_tuning_get(key) for key in KEYS] == [0] * len(KEYS)
