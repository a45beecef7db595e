"""Float64 statements of the per-tensor FP8 path and the RMSNorm quantiser, their inputs, and the CPU models the slacks
of tests/utils.py are measured on (tests/test_normalization_bar.py, tests/test_act_quant_bar.py,
tests/test_group_gemm_pertensor_exact.py), and the statements of the blockwise grouped GEMM's k-block chain and of the MoE
reduce with their float64 emulation of fp32 FMAs (tests/test_group_gemm_blockwise_exact.py, tests/test_moe_reduce_bar.py).
CPU tensors only."""
import functools

import torch

from utils import ACT_SLACK

F8 = torch.float8_e4m3fn


def f32(v):
    """a Python float as the fp32 value a C `float` argument or an fp32 tensor holds, back as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------ RMSNorm
def rmsnorm_ref64(x, w, eps):
    """y = x * rsqrt(mean(x^2) + eps) * w in float64, not rounded; eps as the fp32 value the op's C-ABI receives.  The
    caller multiplies by 1 / scale in float64 and clamps to +-448."""
    x64 = x.double()
    return x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + f32(eps)) * w.double().reshape(1, -1)


NORM_HIDDEN = [8, 320, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 6144, 6152, 8192, 8200, 16384]  # both ends of every rung
NORM_ROWS = [1, 3, 5, 9]            # partial workgroups at 4, 2 and 1 rows per workgroup
NORM_SCALES = [[2.5, 5.0], [0.37, 0.011]]  # the second pair saturates part of the output
NORM_EPS = 1e-6


def norm_lane_vector(hidden):
    """the 16-byte vector that holds the whole energy of the one-lane row: in the second register of its thread where the
    ladder gives a thread more than one, never the first or the last vector of the row"""
    nvec = hidden // 8
    return min(nvec - 1, 256 + 77) if nvec > 256 else (nvec * 5) // 8


@functools.lru_cache(maxsize=None)
def norm_inputs(rows, hidden):
    """-> (x bf16 [rows, hidden], w bf16 [1, hidden]).  Row r is randn * 2^((r mod 5) - 2), so neighbouring rows differ in
    rms, and rows 1 ... 4 are needles: 1 has all its energy in its last 8 elements, 2 in one lane's vector
    (norm_lane_vector), 3 is of magnitude 1e-3 (eps matters), 4 is all zero.  Shared by the tests: never written."""
    g = torch.Generator().manual_seed(rows * 100003 + hidden)
    x = torch.randn(rows, hidden, generator=g) * torch.exp2((torch.arange(rows) % 5 - 2).float()).unsqueeze(1)
    for r, keep in ((1, slice(hidden - 8, hidden)), (2, slice(8 * norm_lane_vector(hidden), 8 * norm_lane_vector(hidden) + 8))):
        if r < rows:
            kept = x[r, keep].clone()
            x[r] = 0
            x[r, keep] = kept
    if rows > 3:
        x[3] = torch.randn(hidden, generator=g) * 1e-3
    if rows > 4:
        x[4] = 0
    w = torch.rand(1, hidden, generator=g) + 0.25
    return x.bfloat16(), w.bfloat16()


def norm_targets(y64, scale):
    """float64 targets of the e4m3 outputs, one per scale: y / scale with the scale's fp32 value, clamped (NaN stays)"""
    return [(y64 * (1.0 / f32(s))).clamp(-448.0, 448.0) for s in scale]


def e4m3_truncate(v):
    """e4m3 cast that rounds toward zero instead of to nearest (a planted error): fp32 -> e4m3 code whose value is the
    largest not above |v|"""
    q = v.float().clamp(-448.0, 448.0).to(F8)
    over = q.float().abs() > v.float().abs()
    b = q.view(torch.uint8).clone()
    b[over] -= 1  # the next code toward zero (sign bit untouched: no code that is over is a zero)
    return b.view(F8)


# ------------------------------------------------------------------------------------- SiLU * up and its quantisation
def silu64(g):
    g64 = g.double()
    return g64 / (1.0 + torch.exp(-g64))


def _bf16_rne(v64):
    """float64 -> bf16, one rounding to nearest even; for values fp32 holds exactly (here: products of two bf16 values)"""
    v32 = v64.float()
    assert bool((v32.double() == v64).all())
    return v32.bfloat16().double()


def silu_mul_ref64(gate_up, use_bf16_mul):
    """a = silu(gate) * up of a bf16 [rows, 2 * inter] tensor in float64.  use_bf16_mul=False: the float64 product, one
    tensor.  use_bf16_mul=True: csrc/act_quant.h::mul_bf16_rounded, bf16(bf16(silu) * up) - the second rounding is of an
    exact 16-bit product, the first is ambiguous where the float64 silu lies within ACT_SLACK * |silu| of a bf16 rounding
    boundary, so both roundings are returned, (a_first, a_second); they are equal wherever the rounding is certain."""
    gate, up = torch.chunk(gate_up, 2, dim=-1)
    s, u = silu64(gate), up.double()
    if not use_bf16_mul:
        return s * u
    # fp32 holds s * (1 -+ slack) to 2^-24: far inside the slack that separates the two candidates
    lo, hi = (s * (1.0 - ACT_SLACK)).float().bfloat16().double(), (s * (1.0 + ACT_SLACK)).float().bfloat16().double()
    return _bf16_rne(lo * u), _bf16_rne(hi * u)


def act_block_scale_ref64(a64):
    """amax / 448 per 128 consecutive columns: [rows, inter] -> [rows, inter / 128]"""
    rows, inter = a64.shape
    return a64.view(rows, inter // 128, 128).abs().amax(-1) / 448.0


EPS_BLOCK = f32(1e-8)  # the 1e-8f of csrc/act_quant.h::e4m3_block_inv


def act_block_targets(a64, scale):
    """float64 targets of the blockwise codes for a given scale [rows, inter / 128]: a / (scale + 1e-8), clamped"""
    return (a64 / (scale.double() + EPS_BLOCK).repeat_interleave(128, dim=1)).clamp(-448.0, 448.0)


def silu_device_model(g, ulps):
    """g / (1 + __expf(-g)) as the device computes it, on the CPU in fp32: the exponential evaluated in float64, rounded
    to fp32 and moved by `ulps` fp32 ulps (the guide states no accuracy for the hardware exponential: +-1 ulp), then
    the add and the divide each rounded to fp32"""
    g32 = g.float()
    e = torch.exp(-g32.double()).float()
    if ulps:  # frexp: e = m * 2^x with m in [0.5, 1), so an ulp of e is 2^(x - 24); 0 and inf stay what they are
        e = torch.where(e.isfinite() & (e > 0), e + ulps * torch.exp2(torch.frexp(e)[1].float() - 24), e)
    return g32 / (1.0 + e)


ACT_EXTREMES = [0.0, -0.0, 90.0, -90.0, 1e4, -1e4, 88.5, -88.5]  # one 8-column chunk; 1e4 is 9984 in bf16
ACT_INTER = [8, 120, 128, 136, 2048, 2056]
ACT_SCALES = [1.7, -0.6, 300.0]
ACT_EXPERTS, ACT_PER_EXPERT, ACT_COUNTS = 4, 48, [0, 48, 1, 47]
ACT_ZERO_ROW, ACT_LASTCOL_ROW = 49, 51  # rows of expert 1, which keeps all of its rows


@functools.lru_cache(maxsize=None)
def act_inputs(rows, inter):
    """-> gate_up bf16 [rows, 2 * inter]: gates randn * 2 clamped to |g| <= 8, ups randn.  Every even row carries
    ACT_EXTREMES in the gates of its last 8 columns with up = +1 (row % 4 == 0) or -1.  With rows > ACT_LASTCOL_ROW and
    inter >= 128: row ACT_ZERO_ROW has up = 0 over its first 128 columns (an all-zero quant block) and row
    ACT_LASTCOL_ROW has the largest product of its first block in column 127.  Shared by the tests: never written."""
    g = torch.Generator().manual_seed(rows * 7919 + inter)
    gate = (torch.randn(rows, inter, generator=g) * 2).clamp(-8.0, 8.0)
    up = torch.randn(rows, inter, generator=g)
    gate[0::2, inter - 8 :] = torch.tensor(ACT_EXTREMES)
    up[0::4, inter - 8 :] = 1.0
    up[2::4, inter - 8 :] = -1.0
    if rows > ACT_LASTCOL_ROW and inter >= 128:
        up[ACT_ZERO_ROW, :128] = 0.0
        gate[ACT_LASTCOL_ROW, 127], up[ACT_LASTCOL_ROW, 127] = 7.5, -9.0
    return torch.cat([gate, up], dim=1).bfloat16()


def act_extreme_mask(rows, inter):
    m = torch.zeros(rows, inter, dtype=torch.bool)
    m[0::2, inter - 8 :] = True
    return m


def act_extreme_expected(gate_up, scale):
    """the planted extremes by value: silu(g) is g for g >= 88.5 and 0 (of either sign) for g <= -88.5 and g = +-0, so the
    output is e4m3(g * u * scale) saturated, or 0; fp32 product as the kernel forms it (g * u is exact, u = +-1)"""
    gate, up = torch.chunk(gate_up.float(), 2, dim=-1)
    v = torch.where(gate > 0, gate * up, torch.zeros_like(gate)) * torch.tensor(scale, dtype=torch.float32)
    return v.clamp(-448.0, 448.0).to(F8).float()


def act_keep_mask():
    r = torch.arange(ACT_EXPERTS * ACT_PER_EXPERT)
    return (r % ACT_PER_EXPERT) < torch.tensor(ACT_COUNTS)[r // ACT_PER_EXPERT]


# --------------------------------------------------------------------------------- per-tensor grouped GEMM, exact inputs
def gemm_exact_inputs(seqlens, n, k, seed, spare_rows=0):
    """-> (x e4m3 [sum(seqlens) + spare_rows, k], w e4m3 [G, n, k]) of integers, x in -3 ... 3 and w in -4 ... 4, so every
    partial sum of x @ w.T is an integer below 12 * k <= 21504 < 2^15: exact in fp32 in any order and any grouping.  Three
    rows in ten of x and of every w[g] share one random sign pattern over k (magnitudes 1 ... 3 and 1 ... 4), the others are
    uniform: where two such rows meet the sum is near 5 * k, so at k = 64 and 128 too there are outputs of more than 8
    significant bits - bf16 ties among them - which uniform integers (|sum| < 256 there) never give."""
    g = torch.Generator().manual_seed(seed)
    total, G = sum(seqlens) + spare_rows, len(seqlens)
    sign = torch.randint(0, 2, (k,), generator=g) * 2 - 1

    def draw(shape, top):
        uniform = torch.randint(-top, top + 1, shape, generator=g)
        aligned = torch.randint(1, top + 1, shape, generator=g) * sign
        return torch.where(torch.rand(shape[:-1], generator=g).unsqueeze(-1) < 0.3, aligned, uniform)

    x, w = draw((total, k), 3), draw((G, n, k), 4)
    return x.float().to(F8), w.float().to(F8)


def group_gemm_pertensor_exact(x, w, seqlens, cu, scale):
    """y[rows of group g] = (x @ w[g].T) * scale[g] in float64: on integer inputs the matmul is exact (every partial sum is
    an integer far below 2^53), the product with the scale's fp32 value is rounded once, to float64."""
    y = torch.zeros((x.shape[0], w.shape[1]), dtype=torch.float64)
    for i in range(w.shape[0]):
        s, cnt = int(cu[i]), int(seqlens[i])
        if cnt:
            y[s : s + cnt] = (x[s : s + cnt].double() @ w[i].double().t()) * scale[i].float().double()
    return y


def bf16_rne64(y64):
    """float64 -> bf16 with ONE rounding to nearest even (through fp32 it would be two): on the bit pattern of the
    float64, 53 - 8 = 45 fraction bits dropped.  Normal results only."""
    b = y64.contiguous().view(torch.int64)
    b = b + ((1 << 44) - 1) + ((b >> 45) & 1)
    return ((b >> 45) << 45).view(torch.float64).float().bfloat16()


def bf16_truncate64(y64):
    """float64 -> bf16 toward zero (a planted error)"""
    return ((y64.contiguous().view(torch.int64) >> 45) << 45).view(torch.float64).float().bfloat16()


def bf16_tie_share(y64):
    """share of the float64 values that sit exactly half way between two bf16 values"""
    b = y64.contiguous().view(torch.int64)
    return float(((b & ((1 << 45) - 1)) == (1 << 44)).double().mean())


# ------------------------------------------------------------------- blockwise grouped GEMM, exact inputs (128-block scales)
LOUD = 2.0 ** 20  # what every scale holds that belongs to no valid (row, k-block) or (n-block, k-block): finite, and never right


def pad4(v):
    return (v + 3) // 4 * 4


def fma32(a64, b64, c64):
    """fp32 fmaf(a, b, c) on float64 tensors that hold fp32 values whose product a * b is exact in float64 (here: 11 x 24
    bits) -> (the fp32 result as float64, mask of the elements where it is not certain).  The float64 sum p + c is rounded
    once; TwoSum recovers its error.  Rounding that sum to fp32 is the one rounding of a true FMA unless the float64 sum was
    inexact AND sits exactly half way between two fp32 values - then the lost bits decide the direction, and the mask says
    so.  (An inexact sum that is no midpoint is at least one float64 ulp from the nearest one: same side as the true sum.)
    Normal fp32 results only."""
    p = a64 * b64
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    mid = (s.contiguous().view(torch.int64) & ((1 << 29) - 1)) == (1 << 28)
    return s.float().double(), mid & (err != 0)


def blockwise_scales(rows, num_group, n, k, seed, kind, loud_rows=None):
    """-> (xs f32 [rows, k / 128], ws f32 [num_group, n / 128, pad4(k / 128)]).  kind "pow2": xs = 2^e, ws = +-2^e with e in
    -3 ... 1; "general": xs = rand + 0.5, ws = +-(rand + 0.5).  The signs are drawn per (group, n-block, k-block) and are the
    same for both kinds.  ws columns kb >= k / 128 and the xs rows named by loud_rows hold LOUD."""
    g = torch.Generator().manual_seed(seed)
    kb = k // 128
    sign = (torch.randint(0, 2, (num_group, n // 128, kb), generator=g) * 2 - 1).float()
    ex, ew = torch.randint(-3, 2, (rows, kb), generator=g), torch.randint(-3, 2, (num_group, n // 128, kb), generator=g)
    rx, rw = torch.rand((rows, kb), generator=g), torch.rand((num_group, n // 128, kb), generator=g)
    xs = torch.exp2(ex.float()) if kind == "pow2" else rx + 0.5
    ws = torch.full((num_group, n // 128, pad4(kb)), LOUD)
    ws[:, :, :kb] = sign * (torch.exp2(ew.float()) if kind == "pow2" else rw + 0.5)
    if loud_rows is not None:
        xs[loud_rows] = LOUD
    return xs.contiguous(), ws


def blockwise_block_sums(x, w, row_group):
    """float64 [k / 128, M, N]: sum_{k in block} x[m, k] * w[row_group[m], n, k].  Integer inputs: computed in fp32, where
    every partial sum is an integer below 2^24 - exact in any order."""
    m, k = x.shape
    n, kb = w.shape[1], k // 128
    x32, parts = x.float().view(m, kb, 128), torch.zeros(kb, m, n, dtype=torch.float64)
    for grp in row_group.unique().tolist():
        rows = torch.nonzero(row_group == grp).flatten()
        parts[:, rows] = torch.einsum("mbk,nbk->bmn", x32[rows], w[grp].float().view(n, kb, 128)).double()
    return parts


def blockwise_chain(parts, xs, ws_rows, form="fma", order=None):
    """The grouped blockwise GEMM's k-block chain on the CPU.  parts float64 [KB, M, N] (blockwise_block_sums), xs
    f32 [M, KB], ws_rows f32 [M, N / 128, KB]: the weight scales each ROW uses.  form "fma": f = fp32(xs * ws), tot =
    fmaf(part, f, tot) over `order` (default ascending) - the statement; "eager": tot += (part * xs) * ws, every operation
    rounded to fp32 (the eager model); "round_product": tot += fp32(part * f).
    -> (tot, the fp32 values as float64 [M, N]; flagged, how many FMAs fma32 could not decide; exact, the float64 sum of
    part * xs * ws; A, the sum of the |terms|; inexact, how many running sums were rounded)."""
    kb, m, n = parts.shape
    tot = torch.zeros(m, n, dtype=torch.float64)
    exact, big_a = torch.zeros_like(tot), torch.zeros_like(tot)
    flagged = inexact = 0
    for b in (range(kb) if order is None else order):
        wsn = ws_rows[:, :, b].repeat_interleave(128, dim=1)  # [M, N]
        xsb = xs[:, b].unsqueeze(1)
        f = (xsb * wsn).double()  # one fp32 multiply
        term = parts[b] * xsb.double() * wsn.double()
        exact, big_a = exact + term, big_a + term.abs()
        if form == "fma":
            true = parts[b] * f + tot
            tot, flag = fma32(parts[b], f, tot)
            flagged += int(flag.sum())
            inexact += int((tot != true).sum())
        elif form == "eager":
            tot = (tot.float() + (parts[b].float() * xsb) * wsn).double()
        else:
            tot = (tot.float() + parts[b].float() * f.float()).double()
    return tot, flagged, exact, big_a, inexact


def xs_transposed(xs, seqlens, cu, tile_m, extra=64):
    """the torch op's activation-scale layout: f32 [KB, sum(ceil(seqlens / tile_m)) * tile_m + extra], group g's rows at
    columns cu_tiles[g] * tile_m ...; every other column holds LOUD"""
    tiles = [(int(c) + tile_m - 1) // tile_m for c in seqlens]
    out = torch.full((xs.shape[1], sum(tiles) * tile_m + extra), LOUD)
    col = 0
    for i, c in enumerate(int(c) for c in seqlens):
        out[:, col : col + c] = xs[int(cu[i]) : int(cu[i]) + c].t()
        col += tiles[i] * tile_m
    return out


def xs_from_transposed(xs_t, seqlens, tile_m):
    """rows [sum(seqlens), KB] read back from xs_transposed's layout with `tile_m` (the wrong one: a planted error)"""
    rows, col = [], 0
    for c in (int(c) for c in seqlens):
        rows.append(xs_t[:, col : col + c].t())
        col += (c + tile_m - 1) // tile_m * tile_m
    return torch.cat(rows).contiguous()


# ---------------------------------------------------------------------------------------------------------- MoE reduce
def moe_reduce_chain(x, pos, scale, shared, skip=True, shared_times=1):
    """csrc/fuse_moe.hip::reduce_kernel on the CPU: acc = fmaf(float(x[pos_j]), scale_j, acc) in j order, pos < 0 skipped
    (skip=False: read as row 0, a planted error), then acc += shared (shared_times of them), every step rounded to fp32.
    -> (acc fp32 values as float64 [T, H]; exact, the float64 sum; A, the sum of the |terms|)."""
    num_tokens, topk = pos.shape
    acc = torch.zeros(num_tokens, x.shape[1], dtype=torch.float64)
    exact, big_a = torch.zeros_like(acc), torch.zeros_like(acc)
    for j in range(topk):
        p = pos[:, j].long()
        on = (p >= 0) if skip else torch.ones_like(p, dtype=torch.bool)
        xr = x[p.clamp_min(0)].double()
        sc = scale[:, j].double().unsqueeze(1)
        term = torch.where(on.unsqueeze(1), xr * sc, torch.zeros_like(xr))  # 8 x 24 bits: exact
        acc = torch.where(on.unsqueeze(1), fma32(xr, sc.expand_as(xr), acc)[0], acc)
        exact, big_a = exact + term, big_a + term.abs()
    for _ in range(shared_times if shared is not None else 0):
        acc = (acc + shared.double()).float().double()  # (through float64: exact on the power-of-two inputs, which alone are held to bits)
        exact, big_a = exact + shared.double(), big_a + shared.double().abs()
    return acc, exact, big_a
