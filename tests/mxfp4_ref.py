"""The statement of the MXFP4-weight grouped GEMM and fused MoE (csrc/group_gemm_mxfp4.hip, csrc/fuse_moe.hip), CPU tensors only:
the formats, the GEMM in float64, the kernel's fp32 k-block chain emulated in float64 (tests/quant_ref.py::fma32), a weight
quantiser for building inputs, and the input builders of tests/test_mxfp4*.py.

  P[r, n, kb] = sum over the 128 k of block kb of  x[r, k] * e2m1(w[g, n, k]) * 2^(s[g, n, k / 32] - 127)
  tot = fmaf(P[r, n, kb], xs[r, kb], tot)      kb ascending, fp32;      y[r, n] = bf16_rne(tot)
"""
import functools
import types

import torch

import quant_ref as qr

F8 = torch.float8_e4m3fn
# OCP e2m1: sign, two exponent bits, one mantissa bit; codes 0 ... 15
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], dtype=torch.float64)


def pack_e2m1(codes, swapped=False):
    """codes uint8 [..., K] in 0 ... 15 -> uint8 [..., K / 2]: the even k in the LOW nibble (swapped: in the high one, a planted error)"""
    lo, hi = (codes[..., 1::2], codes[..., 0::2]) if swapped else (codes[..., 0::2], codes[..., 1::2])
    return (lo | (hi << 4)).to(torch.uint8).contiguous()


def unpack_e2m1(packed, swapped=False):
    """uint8 [..., K / 2] -> the values, float64 [..., K]"""
    lo, hi = (packed & 15).long(), (packed >> 4).long()
    pair = torch.stack((hi, lo) if swapped else (lo, hi), dim=-1)
    return E2M1[pair].reshape(*packed.shape[:-1], packed.shape[-1] * 2)


def e8m0(scale, bias=127):
    """uint8 -> 2^(byte - 127) as float64; byte 255 is NaN"""
    v = torch.exp2(scale.double() - bias)
    return torch.where(scale == 255, torch.full_like(v, float("nan")), v)


def dequant(w, s, per=32, bias=127, swapped=False, roll_rows=0):
    """w uint8 [..., N, K / 2], s uint8 [..., N, K / 32] -> float64 [..., N, K].  per / bias / swapped / roll_rows: planted errors
    (one scale per `per` values read from the same bytes in order, another bias, the nibbles swapped, the scale of the
    neighbouring row)."""
    v = unpack_e2m1(w, swapped)
    k = v.shape[-1]
    sc = e8m0(s, bias)
    if roll_rows:
        sc = sc.roll(roll_rows, -2)
    if per != 32:  # a kernel that takes a group's scale bytes [G, N, K / 32] for [G, N, K / per]: row n reads k / per bytes from n * k / per on
        flat = sc.reshape(sc.shape[0], -1)
        idx = torch.arange(sc.shape[1] * (k // per)) % flat.shape[1]
        sc = flat[:, idx].reshape(sc.shape[0], sc.shape[1], k // per)
    return v * sc.repeat_interleave(per, dim=-1)


def quantise_mxfp4(w):
    """float [..., K] -> (codes packed uint8 [..., K / 2], scales uint8 [..., K / 32]), the OCP MX recipe: per 32 values the shared
    exponent floor(log2(amax)) - 2 (2 = e2m1's largest exponent), values divided by it and rounded to the nearest e2m1 value
    (ties to the even code), saturated at +-6.  An all-zero block gets scale byte 127."""
    k = w.shape[-1]
    blocks = w.double().reshape(*w.shape[:-1], k // 32, 32)
    amax = blocks.abs().amax(-1)
    e = torch.where(amax > 0, torch.floor(torch.log2(amax.clamp_min(1e-300))) - 2, torch.zeros_like(amax)).clamp(-127, 127)
    v = (blocks / torch.exp2(e).unsqueeze(-1)).clamp(-6.0, 6.0)
    mag = E2M1[:8]
    d = (v.abs().unsqueeze(-1) - mag).abs()
    best = d.argmin(-1)
    # a tie between two neighbours goes to the even code: argmin takes the lower one, the upper one is right when it is even
    tie = (d.gather(-1, (best + 1).clamp_max(7).unsqueeze(-1)).squeeze(-1) == d.gather(-1, best.unsqueeze(-1)).squeeze(-1)) & (best < 7)
    best = torch.where(tie & (best % 2 == 1), best + 1, best)
    codes = (best + 8 * (v < 0)).to(torch.uint8).reshape(*w.shape[:-1], k)
    return pack_e2m1(codes), (e + 127).to(torch.uint8).contiguous()


# ---------------------------------------------------------------------------------------------------------------- the GEMM
def block_sums(x, wd, row_group):
    """float64 [K / 128, M, N]: sum over block kb of x[m, k] * wd[row_group[m], n, k], wd the dequantised weights (float64).
    On the exact inputs below every product and partial sum is a multiple of 2^-4 below 2^13: exact in any order."""
    m, k = x.shape
    n, kb = wd.shape[1], k // 128
    x64, parts = x.double().view(m, kb, 128), torch.zeros(kb, m, n, dtype=torch.float64)
    for grp in row_group.unique().tolist():
        rows = torch.nonzero(row_group == grp).flatten()
        parts[:, rows] = torch.einsum("mbk,nbk->bmn", x64[rows], wd[grp].view(n, kb, 128))
    return parts


def statement(parts, xs):
    """-> y float64 [M, N] = sum_kb P[kb] * xs[:, kb]"""
    return torch.einsum("bmn,mb->mn", parts, xs.double())


def chain(parts, xs, form="fma", order=None):
    """the kernel's chain on the CPU: tot = fmaf(P[kb], xs[:, kb], tot), kb ascending (order: another one); form "round_product":
    tot += fp32(P * xs), a rounded product plus a separate add.  parts must hold fp32 values.
    -> (tot as float64 [M, N], FMAs fma32 could not decide, running sums that were rounded)"""
    kb, m, n = parts.shape
    tot = torch.zeros(m, n, dtype=torch.float64)
    flagged = inexact = 0
    for b in (range(kb) if order is None else order):
        f = xs[:, b].double().unsqueeze(1).expand(m, n)
        if form == "fma":
            true = parts[b] * f + tot
            tot, flag = qr.fma32(parts[b], f, tot)
            flagged += int(flag.sum())
            inexact += int((tot != true).sum())
        else:
            tot = (tot.float() + (parts[b] * f).float()).double()
    return tot, flagged, inexact


def gemm_ref(x, xs, w, s, seqlens, cu, rows=None, **planted):
    """the whole statement: -> (y float64 [M, N], A float64: the statement with absolute values everywhere, parts).  rows: the
    row of x / xs each output row reads (row_index), default row for row"""
    total = int(sum(int(c) for c in seqlens))
    group = torch.repeat_interleave(torch.arange(len(seqlens)), torch.as_tensor(seqlens).long())
    rows = torch.arange(total) if rows is None else rows.long()[:total]
    xr, xsr = x.view(torch.uint8)[rows].view(F8), xs[rows]
    wd = dequant(w, s, **planted)
    parts = block_sums(xr.float(), wd, group)
    big_a = torch.einsum("bmn,mb->mn", block_sums(xr.float().abs(), wd.abs(), group), xsr.double().abs())
    return statement(parts, xsr), big_a, parts


def gemm_brute(x, xs, w, s, seqlens, cu):
    """the statement as a plain loop over (group, row, n, k-block, k): Python floats, for tiny shapes"""
    m, k = x.shape
    n = w.shape[1]
    y = torch.zeros(m, n, dtype=torch.float64)
    xf = x.float().tolist()
    for g, cnt in enumerate(int(c) for c in seqlens):
        for r in range(int(cu[g]), int(cu[g]) + cnt):
            for col in range(n):
                acc = 0.0
                for kb in range(k // 128):
                    p = 0.0
                    for kk in range(kb * 128, kb * 128 + 128):
                        byte = int(w[g, col, kk // 2])
                        code = (byte >> 4) if kk % 2 else (byte & 15)
                        p += xf[r][kk] * float(E2M1[code]) * 2.0 ** (int(s[g, col, kk // 32]) - 127)
                    acc += p * float(xs[r, kb])
                y[r, col] = acc
    return y


# ------------------------------------------------------------------------------------------------------------ input builders
def cu_of(seqlens):
    sl = torch.tensor(seqlens, dtype=torch.int32)
    return sl, torch.cat([torch.zeros(1, dtype=torch.int32), torch.cumsum(sl, 0).to(torch.int32)])


def exact_inputs(seqlens, n, k, seed, spare_rows=0):
    """-> namespace: x e4m3 [rows, k] of integers -3 ... 3, w uint8 [G, n, k / 2] of any e2m1 code, s uint8 [G, n, k / 32] with
    2^-3 ... 2^1, xs_pow2 f32 [rows, k / 128] with 2^-3 ... 2^1 and xs_general = rand + 0.5.  Three rows in ten of x and of every
    w[g] share one sign pattern over k with magnitudes away from zero (as tests/quant_ref.py::gemm_exact_inputs has it), so there
    are outputs of more than 8 significant bits, bf16 ties among them."""
    g = torch.Generator().manual_seed(seed)
    G, total = len(seqlens), sum(seqlens) + spare_rows
    sign = torch.randint(0, 2, (k,), generator=g)  # 1 = negative
    xu = torch.randint(-3, 4, (total, k), generator=g)
    xa = torch.randint(1, 4, (total, k), generator=g) * (1 - 2 * sign)
    x = torch.where(torch.rand(total, 1, generator=g) < 0.3, xa, xu).float().to(F8)
    cu_ = torch.randint(0, 16, (G, n, k), generator=g)
    ca = torch.randint(3, 8, (G, n, k), generator=g) + 8 * sign
    codes = torch.where(torch.rand(G, n, 1, generator=g) < 0.3, ca, cu_).to(torch.uint8)
    s = torch.randint(124, 129, (G, n, k // 32), generator=g).to(torch.uint8)
    xs_pow2 = torch.exp2(torch.randint(-3, 2, (total, k // 128), generator=g).float())
    xs_general = torch.rand(total, k // 128, generator=g) + 0.5
    return types.SimpleNamespace(x=x, w=pack_e2m1(codes), codes=codes, s=s, xs={"pow2": xs_pow2, "general": xs_general})


def real_inputs(seqlens, n, k, seed):
    """x, xs: normal data through the 128-block e4m3 quantiser's arithmetic (amax / 448, one multiply by 1 / (scale + 1e-8));
    weights: normal data / sqrt(k), row n times 2^(n % 5 - 2) so that neighbouring rows differ in scale, through quantise_mxfp4"""
    g = torch.Generator().manual_seed(seed)
    total, G = sum(seqlens), len(seqlens)
    a = torch.randn(total, k, generator=g)
    scale = (a.view(total, k // 128, 128).abs().amax(-1) / 448.0).float()
    inv = 1.0 / (scale + 1e-8)
    x = (a * inv.repeat_interleave(128, dim=1)).clamp(-448, 448).to(F8)
    w, s = quantise_mxfp4(torch.randn(G, n, k, generator=g) / k ** 0.5 * torch.exp2((torch.arange(n) % 5 - 2.0)).view(1, n, 1))
    return types.SimpleNamespace(x=x, xs=scale.contiguous(), w=w, s=s)


# ------------------------------------------------------------------------------------------------------------ the fused MoE
def slots(ids, rank_ep, el):
    """stable arrival order (csrc/fuse_moe.hip::slot_kernel): -> (seqlens [el], cu [el + 1], row_index [routed], pos [T, k])"""
    T, topk = ids.shape
    flat = ids.flatten().long() - rank_ep * el
    local = (flat >= 0) & (flat < el)
    sl = torch.bincount(flat[local], minlength=el).to(torch.int32)
    cu = torch.cat([torch.zeros(1, dtype=torch.int32), torch.cumsum(sl, 0).to(torch.int32)])
    pos = torch.full((T * topk,), -1, dtype=torch.int32)
    row_index = torch.zeros(int(sl.sum()), dtype=torch.int32)
    nxt = cu[:-1].clone()
    for i in torch.nonzero(local).flatten().tolist():
        e = int(flat[i])
        pos[i] = nxt[e]
        row_index[int(nxt[e])] = i // topk
        nxt[e] += 1
    return sl, cu, row_index, pos.view(T, topk)


def fuse_moe_ref(x, xs, guw, gus, dw, ds, ids, topk_scale, rank_ep, shared=None, swap_halves=False):
    """the fused op in float64 stage by stage, each stage's output rounded as the device rounds it (bf16 gate-up matrix, e4m3
    activation with fp32 128-block scales, bf16 down output, bf16 result): -> (y float64 before the last rounding, gate_up bf16).
    swap_halves: the activation reads up | gate (a planted error)."""
    el = guw.shape[0]
    sl, cu, row_index, pos = slots(ids, rank_ep, el)
    gu64, _, parts = gemm_ref(x, xs, guw, gus, sl.tolist(), cu, rows=row_index)
    gate_up = chain(parts, xs[row_index.long()])[0].float().bfloat16()
    inter = gate_up.shape[1] // 2
    gu = torch.cat([gate_up[:, inter:], gate_up[:, :inter]], dim=1) if swap_halves else gate_up
    a = (qr.silu_device_model(gu[:, :inter], 0) * gu[:, inter:].float()).float()  # fp32 as csrc/act_quant.h, exp to within an ulp
    scale = (a.view(-1, inter // 128, 128).abs().amax(-1) / 448.0).float()
    q = (a * (1.0 / (scale + 1e-8)).repeat_interleave(128, dim=1)).clamp(-448, 448).to(F8)
    _, _, parts2 = gemm_ref(q, scale, dw, ds, sl.tolist(), cu)
    down = chain(parts2.float().double(), scale)[0].float().bfloat16()
    if down.shape[0] == 0:  # nothing routed to this rank: every pos is -1, the row is never read
        down = torch.zeros(1, down.shape[1], dtype=torch.bfloat16)
    acc, exact, _ = qr.moe_reduce_chain(down, pos, topk_scale, shared)
    return acc, gate_up


@functools.lru_cache(maxsize=8)
def moe_inputs(T, E, topk, rank_ep, size_ep, H, inter, shared, seed=0):
    """exact GEMM inputs for the fused op: x integers, any e2m1 code, power-of-two e8m0 scales, general xs (rand + 0.5)"""
    g = torch.Generator().manual_seed(seed + T * 131 + H + inter)
    el = E // size_ep
    ids = torch.sort(torch.multinomial(torch.ones(T, E), topk, replacement=False, generator=g).to(torch.int32), dim=1)[0]
    a = exact_inputs((T,), 64, H, seed=seed + T + H)
    gu = exact_inputs((1,) * el, 2 * inter, H, seed=seed + T + H + 1)
    dn = exact_inputs((1,) * el, H, inter, seed=seed + T + H + 2)
    sc = torch.rand(T, topk, generator=g)
    sc = sc / sc.sum(1, keepdim=True)
    so = torch.randint(-8, 9, (T, H), generator=g).bfloat16() if shared else None
    return types.SimpleNamespace(x=a.x, xs=a.xs["general"].contiguous(), guw=gu.w, gus=gu.s, dw=dn.w, ds=dn.s, ids=ids, sc=sc, so=so,
                                 el=el)
