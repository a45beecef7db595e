"""Which decode-attention kernel form and grid a call runs: csrc/attention_decode_route.h::decode_route(), a pure host function,
asked through the development build's hpc_dev_decode_route (flat arrays: the members of DecodeCall in, those of DecodeRoute
out).  No GPU: the CU count is part of the call.  The rows are the table of DESIGN 3.2."""
import ctypes
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
OK, UNSUPPORTED, INVALID = 0, -1, -2
ROUTE = ("code", "generation", "mode", "hnd", "share_shift", "passes", "num_nb", "num_wg", "combine_kernel")


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(str(ROOT / "hpc-ops_amd" / "hpc" / "libhpc_amd_dev.so"))
    lib.hpc_dev_decode_route.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    return lib


def call(bf16=False, qt=1, kv=8, group=8, sq=1, page=64, bins=1024, batch=64, lens_on_device=True, cus=256, hnd=False):
    """DecodeCall of a cache in the usual layouts, strides in bytes.  NHD: [page][token][head][128], adjacent heads contiguous;
    HND: [page][head][token][128].  quant_type 0: K-scale rows of 32 floats per head in the page's tail, heads 128 B apart."""
    row = 256 if bf16 else 128
    token, head = (row, row * page) if hnd else (row * kv, row)
    block = row * max(kv, 1) * (page + (4 if not bf16 and qt == 0 else 0))
    ks = (block, 128 * kv, 128) if not bf16 and qt == 0 else (0, 0, 0)
    return [int(bf16), qt, int(lens_on_device), bins, batch, sq, kv * group, kv, page, block, token, head, block, token, head,
            *ks, cus]


def route(lib, c):
    cin = (ctypes.c_int64 * len(c))(*c)
    out = (ctypes.c_int * len(ROUTE))()
    assert lib.hpc_dev_decode_route(cin, len(c), out, len(ROUTE)) == OK
    return dict(zip(ROUTE, out))


def second(mode, share_shift, num_wg, **more):
    return dict(code=OK, generation=2, mode=mode, share_shift=share_shift, num_wg=num_wg, **more)


def first(passes, num_nb, num_wg=1024, **more):
    return dict(code=OK, generation=1, passes=passes, num_nb=num_nb, num_wg=num_wg, **more)


FP8_8x8 = dict(kv=8, group=8)
FP8_4x16 = dict(kv=4, group=16)
BF16_8x8 = dict(bf16=True, kv=8, group=8)
BF16_4x16 = dict(bf16=True, kv=4, group=16)

ROWS = [
    ("fp8_8x8_sq1", dict(**FP8_8x8, sq=1), second(1, 0, 512)),
    ("fp8_8x8_sq2", dict(**FP8_8x8, sq=2), second(1, 0, 512)),
    ("fp8_8x8_sq3", dict(**FP8_8x8, sq=3), second(3, 0, 512)),
    ("fp8_8x8_sq3_page16", dict(**FP8_8x8, sq=3, page=16), first(1, 2)),
    ("fp8_3x8_sq1", dict(kv=3, group=8), first(1, 1)),
    ("fp8_6x4_sq1", dict(kv=6, group=4), second(1, 0, 510)),
    ("fp8_hnd_sq1", dict(**FP8_8x8, hnd=True), first(1, 1)),
    ("fp8_hnd_sq3", dict(**FP8_8x8, hnd=True, sq=3), second(3, 0, 512, hnd=0)),
    ("fp8_qt0_sq1", dict(**FP8_8x8, qt=0), second(1, 0, 512)),
    ("fp8_4x16_sq1", dict(**FP8_4x16, sq=1), second(1, 0, 512)),
    ("fp8_4x16_sq2", dict(**FP8_4x16, sq=2), second(3, 0, 512)),
    ("fp8_4x16_sq3_sliced", dict(**FP8_4x16, sq=3), second(3, 1, 512)),
    ("fp8_4x16_sq3_page16", dict(**FP8_4x16, sq=3, page=16), first(2, 2)),
    ("bf16_8x8_sq1", dict(**BF16_8x8, sq=1), second(1, 0, 512)),
    ("bf16_8x8_sq5", dict(**BF16_8x8, sq=5), first(1, 3)),
    ("bf16_4x16_sq3", dict(**BF16_4x16, sq=3), first(1, 3)),
    ("bf16_4x16_sq4", dict(**BF16_4x16, sq=4), second(3, 1, 512)),
    ("bf16_4x16_sq5", dict(**BF16_4x16, sq=5), first(2, 3)),
    ("bf16_host_lengths", dict(**BF16_8x8, lens_on_device=False), first(1, 1)),
    ("fp8_two_bins", dict(**FP8_8x8, bins=2), first(1, 1, num_wg=2)),
    ("fp8_counters_exceed_64k", dict(kv=64, group=1, batch=1024), first(1, 1, combine_kernel=1)),
    ("fp8_sq5", dict(**FP8_8x8, sq=5), dict(code=UNSUPPORTED)),
    ("fp8_qt0_page16", dict(**FP8_8x8, qt=0, page=16), dict(code=UNSUPPORTED)),
    ("group3", dict(kv=8, group=3), dict(code=UNSUPPORTED)),
    ("no_kv_heads", dict(kv=0, group=8), dict(code=INVALID)),
]

# (development key, value) on one of the calls above
KEY_ROWS = [
    ("key12_first_generation", (12, 1), dict(**FP8_8x8), dict(generation=1)),
    ("key28_bf16_first_generation", (28, 1), dict(**BF16_8x8), dict(generation=1)),
    ("key29_four_heads", (29, 2), dict(**FP8_8x8), second(2, 0, 512)),
    ("key60_never_one_head", (60, 1), dict(**FP8_8x8, sq=3), first(1, 2)),
    ("key60_one_head_odd_heads", (60, 2), dict(kv=3, group=8), second(3, 0, 510)),
    ("key55_hnd_pairs", (55, 1), dict(**FP8_8x8, hnd=True), second(1, 0, 512, hnd=1)),
    ("key14_grid", (14, 64), dict(**FP8_8x8), dict(generation=2, num_wg=64)),
    ("key54_qt0_first_generation", (54, 1), dict(**FP8_8x8, qt=0), dict(generation=1)),
    ("key33_combine_kernel", (33, 1), dict(kv=3, group=8), first(1, 1, combine_kernel=1)),
]


def check(got, want):
    assert {k: got[k] for k in want} == want, got


@pytest.mark.parametrize("name,kw,want", ROWS, ids=[r[0] for r in ROWS])
def test_decode_route(lib, name, kw, want):
    check(route(lib, call(**kw)), want)


@pytest.mark.parametrize("name,key,kw,want", KEY_ROWS, ids=[r[0] for r in KEY_ROWS])
def test_decode_route_development_key(lib, name, key, kw, want):
    assert lib.hpc_dev_tuning_set(key[0], key[1]) == 0
    try:
        check(route(lib, call(**kw)), want)
    finally:
        assert lib.hpc_dev_tuning_set(key[0], 0) == 0


def test_no_device_is_first_generation(lib):
    """a CU count <= 0 (no device to ask) routes what the head-pair form would take to the first generation"""
    check(route(lib, call(**FP8_8x8, cus=0)), first(1, 1))


def test_marshalling_is_checked(lib):
    c = call(**FP8_8x8)
    cin = (ctypes.c_int64 * len(c))(*c)
    out = (ctypes.c_int * len(ROUTE))()
    assert lib.hpc_dev_decode_route(cin, len(c) - 1, out, len(ROUTE)) == INVALID
    assert lib.hpc_dev_decode_route(cin, len(c), out, len(ROUTE) - 1) == INVALID
