"""Scratch buffers: every caller-provided buffer has one layout function that its sizer, its launcher and the torch op read
(DESIGN "scratch buffers").  CPU: the sizes the library reports equal the arithmetic they replaced, kept here as the oracle.
GPU: a buffer of exactly the reported size, between two guard bands, is enough - the carve stays inside what the sizer said."""
import ctypes
import functools
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
GUARD = 1 << 20  # bytes on either side of the scratch
PATTERN = 0xA5


@pytest.fixture(scope="module")
def lib():
    from hpc import _C

    return _C.lib


# ---- the arithmetic the layout functions replaced --------------------------------------------------------------------------------
def old_task_workspace_bytes(num_cu, max_num_batch, max_seqlen, num_head_kv, min_process_len):
    k_task, k_max_cta, k_tile = 48, 4, 64
    max_cta = num_cu * k_max_cta
    total_tiles = max_num_batch * num_head_kv * ((max_seqlen + k_tile - 1) // k_tile)
    max_tasks = 0
    for cta_per_cu in (4, 3, 2, 1):
        ctas = num_cu * cta_per_cu
        per = max((total_tiles + ctas - 1) // ctas, min_process_len // k_tile)
        max_tasks = max(max_tasks, (per + 1) * ctas + 1)
    chunk_bytes = (max_num_batch * num_head_kv * 4 + k_task - 1) // k_task * k_task
    cta_pad = (max_cta + 11) // 12 * 12 * 4
    sched = max_tasks * k_task + chunk_bytes
    return sched + 2 * cta_pad, sched


def old_decode_workspace_bytes(num_bins, num_batch, num_head_kv, num_seq_q, group):
    rows = (num_seq_q * group + 15) // 16 * 16
    first = num_bins * 2 * rows * 128 * 4 + num_bins * 2 * rows * 4 + (num_batch * num_head_kv * 4 + 15) // 16 * 16
    second = num_bins * 2 * 2 * 16 * 128 * 4 + num_bins * 2 * 2 * 16 * 4
    return 64 * 1024 + first + second


def old_router_splits(m, n, k, use_splitk, cus):
    if not use_splitk:
        return 1
    s = 1
    if m <= 256:
        tm = 16 if m <= 16 else (32 if m <= 32 else 64)
        tiles = (m + tm - 1) // tm * (n // 16)
        while s < 16 and tiles * s < cus and (k >> 6) // (s * 2) >= 4:
            s *= 2
        return s
    tiles = (m + 127) // 128 * (n // 64)
    while s < 8 and tiles * s < cus and k // (s * 2) >= 256:
        s *= 2
    if cus <= tiles < 2 * cus and s == 1 and k >= 512:
        s = 2
    return s


def old_router_flags(m, n):
    if m <= 256:
        tm = 16 if m <= 16 else (32 if m <= 32 else 64)
        return (m + tm - 1) // tm, n // 16
    return (m + 63) // 64, n // 64


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_task_workspace_bytes_equal_the_old_arithmetic(lib):
    import hpc.attention

    n = 0
    for cus in (1, 64, 256, 304):
        for batch in (1, 7, 64, 4096):
            for seq in (1, 63, 64, 65, 131072):
                for kv in (1, 3, 8):
                    for mpl in (0, 64, 512, 4096):
                        want = old_task_workspace_bytes(cus, batch, seq, kv, mpl)
                        sched = ctypes.c_int64(-1)
                        total = lib.hpc_attention_decode_task_workspace_bytes(cus, batch, seq, kv, mpl, ctypes.byref(sched))
                        assert (total, sched.value) == want, (cus, batch, seq, kv, mpl)
                        assert hpc.attention.task_workspace_bytes(cus, batch, seq, kv, mpl) == want
                        assert lib.hpc_attention_decode_task_workspace_bytes(cus, batch, seq, kv, mpl, None) == total
                        n += 1
    assert n == 4 * 4 * 5 * 3 * 4
    assert lib.hpc_attention_decode_task_workspace_bytes(0, 1, 64, 1, 0, None) < 0


def test_task_rows_and_workspace_share_the_plan_size(lib):
    """The workspace's scheduler part is the largest plan of the largest batch, in 48-byte records: at one bin count per CU it is
    exactly the rows hpc_assign_attention_decode_task_rows reports for that batch."""
    for cus, batch, seq, kv, mpl in ((64, 7, 4097, 3, 512), (256, 64, 131072, 8, 0), (304, 1, 63, 1, 4096)):
        lens = (ctypes.c_int * batch)(*([seq] * batch))
        rows = max(lib.hpc_assign_attention_decode_task_rows(lens, cus * per_cu, batch, kv, 1, 1, mpl) for per_cu in (1, 2, 3, 4))
        sched = ctypes.c_int64(0)
        lib.hpc_attention_decode_task_workspace_bytes(cus, batch, seq, kv, mpl, ctypes.byref(sched))
        assert sched.value == rows * 48


def test_decode_workspace_bytes_equal_the_old_arithmetic(lib):
    for bins in (1, 64, 256, 512):
        for batch in (1, 64, 1024):
            for kv in (1, 3, 8, 16):
                for sq in range(1, 6):
                    for group in range(1, 17):
                        assert lib.hpc_attention_decode_workspace_bytes(bins, batch, kv, sq, group) == \
                            old_decode_workspace_bytes(bins, batch, kv, sq, group), (bins, batch, kv, sq, group)
    assert lib.hpc_attention_decode_workspace_bytes(0, 1, 1, 1, 1) < 0


def test_router_plan_equals_the_old_rules(lib):
    cus = lib.hpc_get_cu_count(-1)
    cus = cus if cus > 0 else 256  # no device: the library assumes 256
    for m in list(range(1, 301)) + [1024, 4096, 12303]:
        for n in (64, 192, 512, 2048):
            for k in (64, 512, 4096, 7168):
                for use_splitk in (0, 1):
                    splits, rows, ld = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
                    rc = lib.hpc_gemm_bf16xfp32_plan(m, n, k, use_splitk, ctypes.byref(splits), ctypes.byref(rows), ctypes.byref(ld))
                    assert rc == 0, (m, n, k)
                    assert splits.value == lib.hpc_gemm_bf16xfp32_splits(m, n, k, use_splitk), (m, n, k, use_splitk)
                    assert splits.value == old_router_splits(m, n, k, use_splitk, cus), (m, n, k, use_splitk)
                    assert (rows.value, ld.value) == old_router_flags(m, n), (m, n, k)
    one = ctypes.c_int(0)
    assert lib.hpc_gemm_bf16xfp32_plan(8, 64, 96, 1, ctypes.byref(one), ctypes.byref(one), ctypes.byref(one)) == -1  # k % 64
    assert lib.hpc_gemm_bf16xfp32_plan(8, 64, 64, 1, None, ctypes.byref(one), ctypes.byref(one)) == -2


def test_group_gemm_scan_wanted_above_20_rows_per_group(lib):
    for groups in (1, 8, 64):
        for m in range(16 * groups - 1, 22 * groups + 2):
            assert lib.hpc_group_gemm_scan_wanted(groups, m) == int(m // groups > 20), (groups, m)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
def _guarded(nbytes):
    """uint8 [GUARD + nbytes + GUARD] filled with PATTERN; returns (whole buffer, the middle)."""
    buf = torch.full((2 * GUARD + nbytes,), PATTERN, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_untouched(buf, nbytes):
    return bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + nbytes:] == PATTERN).all())


@pytest.mark.gpu
@pytest.mark.parametrize("heads,shape", [((8, 64), "NHD"), ((4, 32), "HND")])
def test_decode_scratch_of_exactly_the_reported_size(lib, heads, shape):
    """fp8 decode through the C entry (the pattern of test_attn_fp8_stale_arrival_counter_is_reported) with a workspace of exactly
    hpc_attention_decode_workspace_bytes bytes between two guard bands: 8 / 64 heads on NHD pages run the second generation,
    4 / 32 on HND pages the first, where the task map splits the long request.  The op's own result bit for bit, the counter region
    zero afterwards, both guards untouched."""
    import hpc
    from hpc import _C
    from test_attention_decode_fp8 import _case

    num_head_kv, num_head_q = heads
    lens = torch.tensor([8192, 3, 130], dtype=torch.int32)
    B, bs = len(lens), 64
    q8, q_scale, kv, block_ids, nblocks = _case(B, 1, lens, bs, heads, False)
    kv_dev = kv.to(torch.float8_e4m3fn).cuda()
    if shape == "HND":
        kv_dev = kv_dev.view(torch.uint8).permute(0, 1, 3, 2, 4).contiguous().permute(0, 1, 3, 2, 4).view(torch.float8_e4m3fn)
    kc, vc = kv_dev[:, 0], kv_dev[:, 1]
    qd, bd, lens_in, qs = q8.cuda(), block_ids.cuda(), (lens + 1).cuda(), q_scale.cuda()
    ks, vs = torch.rand(1).cuda() + 0.5, torch.rand(1).cuda() + 0.5
    task_map = hpc.get_attention_decode_task_workspace(B, int(lens.max()) + 1, num_head_kv)
    hpc.assign_attention_decode_task(lens_in, task_map, num_head_kv, 1, True)
    max_chunks = int(task_map.view(torch.int32)[5])
    print("max chunks of a request:", max_chunks)
    assert max_chunks > 1  # the task map splits the long request: the first generation merges its partials
    want = hpc.attention_decode_fp8(qd, kc, vc, bd, lens_in, qs, ks, vs, mtp=0, new_kv_included=True,
                                    quant_type=hpc.QuantType.QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR, splitk=True,
                                    task_map=task_map)
    torch.cuda.synchronize()
    nbins = lib.hpc_attention_decode_num_bins(1, torch.cuda.current_device())
    zero_bytes = lib.hpc_attention_decode_workspace_zero_bytes()
    nbytes = lib.hpc_attention_decode_workspace_bytes(nbins, B, num_head_kv, 1, num_head_q // num_head_kv)
    assert nbytes > zero_bytes
    buf, ws = _guarded(nbytes)
    ws[:zero_bytes].zero_()

    def ip(t):
        return ctypes.cast(t.data_ptr(), _C.IP)

    y = torch.full_like(want, float("nan"))
    rc = lib.hpc_attention_decode_fp8_async(
        y.data_ptr(), ws.data_ptr(), ip(task_map), qd.data_ptr(), kc.data_ptr(), vc.data_ptr(), ip(bd), ip(lens_in),
        qs.data_ptr(), ks.data_ptr(), vs.data_ptr(), 1, 1, nbins, B, 1, num_head_q, num_head_kv, 128, 128, bs,
        bd.shape[1], qs.stride(0), y.stride(0), qd.stride(0), kc.stride(0), kc.stride(1), kc.stride(2), vc.stride(0),
        vc.stride(1), vc.stride(2), 0, 0, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert _guards_untouched(buf, nbytes)
    assert torch.equal(y, want)
    assert int(ws[:zero_bytes].view(torch.int32).abs().sum()) == 0


@functools.lru_cache(maxsize=None)
def _router_problem(n, k):
    import router_gemm_ref as rr
    from oracle import gemm as orc

    g = torch.Generator().manual_seed(10086)
    x = torch.randn(257, k, generator=g).bfloat16()
    w = torch.randn(n, k, generator=g)
    wh, wl = orc.split_weight(w, 1 / 256)
    return x, wh, wl, rr.ref64(x, wh, wl, 1 / 256), wh.cuda(), wl.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("m", [16, 17, 32, 33, 256, 257])
def test_router_gemm_split_flag_of_exactly_the_planned_size(lib, m):
    """The op with a caller's split_flag of exactly the planned rows x row stride (flat up to 256 tokens, 2-D above) between two
    guard bands, at the edges of the tile ladder: the derived fp32 bar against the two-plane statement (tests/router_gemm_ref.py),
    flags zero after the call, guards untouched."""
    import hpc
    import router_gemm_ref as rr

    n, k = 192, 4096
    x, _, _, (r, big_a), whd, wld = _router_problem(n, k)
    splits, rows, ld = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert lib.hpc_gemm_bf16xfp32_plan(m, n, k, 1, ctypes.byref(splits), ctypes.byref(rows), ctypes.byref(ld)) == 0
    print("m", m, "splits", splits.value, "counter rows", rows.value, "row stride", ld.value)
    assert splits.value > 1  # the counters are in use
    nbytes = rows.value * ld.value * 4
    buf, mid = _guarded(nbytes)
    mid.zero_()
    flag = mid.view(torch.int32)
    if m > 256:
        flag = flag.view(rows.value, ld.value)
    my = hpc.gemm_bf16xfp32(x[:m].cuda(), whd, wld, 1 / 256, True, True, flag)
    torch.cuda.synchronize()
    assert _guards_untouched(buf, nbytes)
    assert rr.close(my.cpu(), r[:m], big_a[:m], f"m {m}")
    assert int(flag.abs().sum()) == 0
