"""Which grouped FP8 GEMM kernel a call runs, in which form and on which grid: csrc/group_gemm_route.h::ggemm_route(), a pure host
function, asked through the development build's hpc_dev_ggemm_route (flat arrays: the members of GgemmCall in, those of
GgemmRoute out).  No GPU.  The rows are the table of DESIGN 3.3."""
import ctypes
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
OK, UNSUPPORTED, INVALID = 0, -1, -2
STREAM, TILED128, RING, P8 = 1, 2, 3, 4
ROUTE = ("code", "kernel", "act", "grid_x", "grid_y", "threads", "mt", "loop", "tile_tokens", "k_tail", "no_dma", "loop_variant",
         "no_half_tile", "nt_single", "tail_regs", "item_scan_old", "ext_rows", "item_order")
KEYS = (1, 3, 6, 18, 19, 21, 22, 23, 24, 25, 26, 43, 49, 56)  # every key ggemm_route() reads


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(str(ROOT / "hpc-ops_amd" / "hpc" / "libhpc_amd_dev.so"))
    lib.hpc_dev_ggemm_route.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    return lib


def call(m, n=512, k=512, G=8, pertensor=False, want_act=False, scan=True):
    """GgemmCall: 8 groups, blockwise scales, n = k = 512 and the scan of ceil(seqlens / 128) present unless said otherwise"""
    return [int(not pertensor), int(want_act), G, m, n, k, int(scan)]


def route(lib, c):
    cin = (ctypes.c_int64 * len(c))(*c)
    out = (ctypes.c_int * len(ROUTE))()
    assert lib.hpc_dev_ggemm_route(cin, len(c), out, len(ROUTE)) == OK
    return dict(zip(ROUTE, out))


def stream(mt, loop=None, grid=None, threads=None):
    want = dict(code=OK, kernel=STREAM, mt=mt)
    if loop is not None:
        want["loop"] = loop
    if grid:
        want.update(grid_x=grid[0], grid_y=grid[1])
    if threads:
        want["threads"] = threads
    return want


def tiled128(grid=None):
    return dict(code=OK, kernel=TILED128, threads=256, **(dict(grid_x=grid[0], grid_y=grid[1]) if grid else {}))


def ring(grid, tokens=128):
    return dict(code=OK, kernel=RING, grid_x=grid, threads=512, tile_tokens=tokens)


def p8(grid=None, **more):
    return dict(code=OK, kernel=P8, threads=512, **(dict(grid_x=grid) if grid else {}), **more)


PT = dict(pertensor=True)

# all keys 0: what the product runs
ROWS = [
    ("avg8", dict(m=64), stream(1, 0, (8, 8), 256)),
    ("avg10", dict(m=80), stream(1)),
    ("avg11", dict(m=88), stream(2)),
    ("avg15", dict(m=120), stream(2, 0)),
    ("avg16", dict(m=128), p8(32, k_tail=0, act=0, ext_rows=1, nt_single=1, item_order=0, no_half_tile=0)),
    ("avg16_n384", dict(m=128, n=384), stream(2, grid=(6, 8))),
    ("avg21_n384", dict(m=168, n=384), tiled128((3, 9))),
    ("avg21_n384_no_scan", dict(m=168, n=384, scan=False), stream(2)),
    ("avg23_n384_no_scan", dict(m=184, n=384, scan=False), stream(3, 1, (6, 8))),
    ("pertensor_n192", dict(**PT, m=320, n=192, k=128), stream(3, grid=(3, 8))),
    ("pertensor_k64", dict(**PT, m=256, n=256, k=64), tiled128((2, 10))),
    ("pertensor_k192", dict(**PT, m=256, n=256, k=192), p8(25, k_tail=1)),
    ("act_avg16", dict(m=128, want_act=True), p8(32, act=1)),
    ("act_avg15", dict(m=120, want_act=True), dict(act=0, **stream(2))),
    ("act_pertensor_k192", dict(**PT, m=128, k=192, want_act=True), p8(act=0, k_tail=1)),
    ("three_rows", dict(m=3), stream(1)),
    ("items_above_2g", dict(G=1, m=1 << 24, n=1 << 23, k=128), dict(code=UNSUPPORTED)),
]

# {development key: value}, then the call
KEY_ROWS = [
    ("key3_never_tiled", {3: 1}, dict(m=2400), stream(3)),
    ("key3_ring", {3: 2}, dict(m=32), ring(24)),
    ("key3_ring_n384", {3: 2}, dict(m=32, n=384), tiled128((3, 8))),
    ("key3_tiled128", {3: 3}, dict(m=128), tiled128((4, 9))),
    ("key3_p8", {3: 4}, dict(m=8), p8(32)),
    ("key3_p8_n384", {3: 4}, dict(m=8, n=384), tiled128()),
    ("key25_ring", {25: 1}, dict(m=800), ring(36)),
    ("key25_p8_from_192", {25: 1}, dict(m=1536), p8(44)),
    ("key6_ring_32", {25: 1, 6: 2}, dict(m=800), ring(120, 32)),
    ("key6_ring_64", {25: 1, 6: 3}, dict(m=800), ring(64, 64)),
    ("key1_form8", {1: 8}, dict(m=64), stream(8, grid=(4, 8), threads=256)),
    ("key1_form16", {1: 16}, dict(m=64), stream(16, grid=(4, 8), threads=512)),
    ("key1_form32", {1: 32}, dict(m=64), stream(32, grid=(4, 8), threads=512)),
    ("key1_form4", {1: 4}, dict(m=64), stream(4, 1, (8, 8))),
    # a forced form of 128-row workgroups at n % 128 != 0 falls through to 32 tokens per pass
    ("key1_form8_n192", {1: 8}, dict(**PT, m=64, n=192, k=128), stream(2, 1, (3, 8))),
    ("key56_old_loop", {56: 1}, dict(m=64), stream(1, 1)),
    ("key56_k32_loop", {56: 2}, dict(m=64), stream(1, 2)),
    ("key56_k32_loop_mt3", {56: 2}, dict(m=184, n=384, scan=False), stream(3, 1)),
    ("key21", {21: 2}, dict(m=128), p8(no_half_tile=2)),
    ("key23", {23: 1}, dict(m=128), p8(item_order=1)),
    ("key24", {24: 1}, dict(m=128), p8(nt_single=0)),
    ("key26", {26: 1}, dict(m=128), p8(tail_regs=1)),
    ("key43", {43: 1}, dict(m=128), p8(item_scan_old=1)),
    ("key49", {49: 1}, dict(m=128), p8(ext_rows=0)),
    ("key22_blockwise", {22: 2}, dict(m=128), p8(loop_variant=2)),
    ("key22_pertensor", {22: 2}, dict(**PT, m=128), p8(loop_variant=0)),
    ("key22_unknown", {22: 5}, dict(m=128), dict(code=INVALID)),
    ("key18", {18: 1}, dict(m=128), p8(no_dma=1)),
    ("key18_act", {18: 1}, dict(m=128, want_act=True), p8(no_dma=0)),
    ("key18_pertensor", {18: 1}, dict(**PT, m=128), p8(no_dma=0)),
    ("key19_split_act", {19: 1}, dict(m=128, want_act=True), p8(act=0)),
]


def check(got, want):
    assert {k: got[k] for k in want} == want, got


@pytest.mark.parametrize("name,kw,want", ROWS, ids=[r[0] for r in ROWS])
def test_ggemm_route(lib, name, kw, want):
    check(route(lib, call(**kw)), want)


@pytest.mark.parametrize("name,keys,kw,want", KEY_ROWS, ids=[r[0] for r in KEY_ROWS])
def test_ggemm_route_development_key(lib, name, keys, kw, want):
    for key, value in keys.items():
        assert lib.hpc_dev_tuning_set(key, value) == 0
    try:
        check(route(lib, call(**kw)), want)
    finally:
        for key in keys:
            assert lib.hpc_dev_tuning_set(key, 0) == 0
    assert [lib.hpc_dev_tuning_get(key) for key in KEYS] == [0] * len(KEYS)


def test_a_refusal_sets_nothing_else(lib):
    got = route(lib, call(G=1, m=1 << 24, n=1 << 23, k=128))
    assert got.pop("code") == UNSUPPORTED and not any(got.values()), got


def test_marshalling_is_checked(lib):
    c = call(m=64)
    cin = (ctypes.c_int64 * len(c))(*c)
    out = (ctypes.c_int * len(ROUTE))()
    assert lib.hpc_dev_ggemm_route(cin, len(c) - 1, out, len(ROUTE)) == INVALID
    assert lib.hpc_dev_ggemm_route(cin, len(c), out, len(ROUTE) - 1) == INVALID
    assert lib.hpc_dev_ggemm_route(None, len(c), out, len(ROUTE)) == INVALID


def test_keys_are_zero_after_the_key_rows(lib):
    """every key row puts its keys back (a key left set would re-route the GPU tests of the same process)"""
    assert [lib.hpc_dev_tuning_get(key) for key in KEYS] == [0] * len(KEYS)
