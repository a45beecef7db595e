"""The statement of hpc.gemm_bf16xfp32 (the router GEMM, csrc/gemm_bf16xfp32.hip) in float64, the builders of its test inputs,
the bar for general inputs, a float32 model of the kernels' summation order and the planted errors the bars must reject.
CPU tensors only; the cached builders' results are shared between tests and must not be written."""
import functools

import torch

from oracle import gemm as orc
from utils import ulp_bf16

EPS24 = 2.0 ** -24  # half an fp32 ulp of a value in [1, 2): one fp32 rounding of a magnitude A costs at most EPS24 * A


def ref64(x, wh, wl, scale):
    """x bf16 [m, k], wh / wl bf16 [n, k] -> (r, A), both float64 [m, n]:
        r[m, n] = sum_k x[m, k] * wh[n, k] + scale * sum_k x[m, k] * wl[n, k]
        A[m, n] = sum_k |x[m, k]| * (|wh[n, k]| + scale * |wl[n, k]|)
    scale enters with its fp32 value, as the kernel receives it.  r is NOT rounded; A bounds every magnitude an fp32 evaluation
    adds up, in any order."""
    assert x.device.type == "cpu" and x.dtype == wh.dtype == wl.dtype == torch.bfloat16 and wh.shape == wl.shape
    s = float(torch.tensor(scale, dtype=torch.float32))
    xd, hd, ld = x.double(), wh.double(), wl.double()
    r = xd @ hd.t() + s * (xd @ ld.t())
    return r, xd.abs() @ (hd.abs() + s * ld.abs()).t()


# ---- exact inputs ------------------------------------------------------------------------------------------------------------------
def exact_ranges(k, scale=1.0 / 256):
    """(max |x|, max |w_high|, max |w_low|) of the exact inputs.  Up to k = 1024: 3, 4, 8.  Above, the sums grow past the sizes
    where one output in a hundred is a bf16 tie (measured with 3, 4, 8: 5 % at k = 64, 2 % at 576, 1.2 % at 2112, 0.9 % at
    4096), so x and w_high narrow to 2 (2 % at 2112 and at 4096); a scale below 1 / 256 adds bits below the point and halves
    the share, so it narrows them too."""
    return (3, 4, 8) if k <= 1024 and scale >= 1.0 / 256 else (2, 2, 8)


@functools.lru_cache(maxsize=None)
def exact_inputs(m, n, k, scale=1.0 / 256, seed=0):
    """-> (x [m, k], w_high [n, k], w_low [n, k]) bf16, small integers within exact_ranges(k); scale a power of two <= 1.  Three
    rows in ten of each tensor share one random sign pattern over k (magnitudes from 1 up), the others are uniform: where such
    rows meet, the sum is near its largest, so small k has outputs of more than 8 significant bits too.  Every product and every
    partial sum, in any order and any split, is a multiple of scale below 2^24 * scale - the bound asserted here - and so exact
    in fp32: the fp32 output must equal float32(r) bit for bit, the bf16 output bf16(r) rounded to nearest even."""
    assert 0 < scale <= 1 and float(torch.frexp(torch.tensor(float(scale)))[0]) == 0.5, scale  # a power of two
    tx, th, tl = exact_ranges(k, scale)
    assert k * tx * (th + scale * tl) / scale < 2.0 ** 24, (k, scale)
    g = torch.Generator().manual_seed(seed * 1000003 + m * 7919 + n * 31 + k)
    sign = torch.randint(0, 2, (k,), generator=g) * 2 - 1

    def draw(rows, top):
        uniform = torch.randint(-top, top + 1, (rows, k), generator=g)
        aligned = torch.randint(1, top + 1, (rows, k), generator=g) * sign
        return torch.where(torch.rand(rows, generator=g).unsqueeze(-1) < 0.3, aligned, uniform).float().bfloat16()

    return draw(m, tx), draw(n, th), draw(n, tl)


def is_bf16_tie(r32):
    """Elements of a float32 tensor that lie exactly half way between two bf16 values."""
    return (r32.contiguous().view(torch.int32) & 0xFFFF) == 0x8000


def bf16_truncated(r32):
    """float32 -> bf16 by dropping the low 16 bits (the planted truncating cast)."""
    return (r32.contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


MIN_TIE_SHARE = 0.01


@functools.lru_cache(maxsize=None)
def exact_case(m, n, k, scale=1.0 / 256):
    """-> (x, w_high, w_low, want32, want16, tie share): exact inputs, float32(r) - asserted to be r -, its bf16 rounding to
    nearest even and the share of outputs that are bf16 ties.  The inputs are those of the first seed whose statement has at
    least MIN_TIE_SHARE ties (a single token row of 64 outputs has none under some seeds); the choice reads the statement alone."""
    for seed in range(16):
        x, wh, wl = exact_inputs(m, n, k, scale, seed)
        r, _ = ref64(x, wh, wl, scale)
        want32 = r.float()
        assert torch.equal(want32.double(), r)
        share = float(is_bf16_tie(want32).float().mean())
        if share >= MIN_TIE_SHARE:
            return x, wh, wl, want32, want32.bfloat16(), share
    raise AssertionError(f"no seed gives {MIN_TIE_SHARE} bf16 ties at {(m, n, k, scale)}")


# ---- real inputs and their bar ---------------------------------------------------------------------------------------------------
REAL_SCALE = 1.0 / 256


@functools.lru_cache(maxsize=None)
def real_inputs(m, n, k, seed=0):
    """-> (x, w_high, w_low, r, A): randn x as bf16, a randn fp32 weight split into its two planes at scale 1 / 256."""
    g = torch.Generator().manual_seed(seed * 1000003 + m * 7919 + n * 31 + k + 5)
    x = torch.randn(m, k, generator=g).bfloat16()
    wh, wl = orc.split_weight(torch.randn(n, k, generator=g), REAL_SCALE)
    return (x, wh, wl) + ref64(x, wh, wl, REAL_SCALE)


RGEMM_SLACK = 4.0
"""fp32 slack of the router GEMM's bar for general inputs (excess / close below), in units of 2^-24 * A per element.

Measured: fp32_model - the kernels' summation order restated in float32 - against the float64 statement on the real-input
cases of tests/test_gemm_bf16xfp32_exact.py, (17, 64, 4096), (33, 64, 2112), (64, 128, 7168) with 4 wave accumulators and
(300, 64, 4096) with one, each at splits 1, 3 / 5, 8 and 16 (the caller's counts and the library's own), has a worst excess of
0.643 x 2^-24 A on the fp32 output (the unsplit single accumulator; 0.13 ... 0.33 everywhere else) and of 0.103 beyond half an
ulp on the bf16 output (test_fp32_model_passes_and_its_excess_holds_the_slack measures it again, prints it and holds the
constant to it; a probe at k 512 ... 7168 gave 0.86).  4 x 0.643 = 2.57, rounded up to a power of two, is 4.  The margin is for what a correct kernel may order
differently: the sum inside a 32-k matrix instruction, the deal of steps to accumulators, a multiply and an add where the model
fuses `acc_l * scale + acc_h`.  Cap: 16; a kernel that needs more is a finding."""
RGEMM_SLACK_CAP = 16.0


def excess(y, r, a):
    """What an output misses the statement by, beyond the rounding of its own type, in units of 2^-24 * A per element:
    (|y - r| - half_ulp_out(r)) / (2^-24 A).  The half-ulp term is bf16's for a bf16 output; an fp32 output has none.  NaN in y
    counts as an infinite excess."""
    assert r.dtype == torch.float64 and y.shape == r.shape and y.dtype in (torch.float32, torch.bfloat16), (y.dtype, y.shape)
    half = 0.5 * ulp_bf16(r) if y.dtype == torch.bfloat16 else torch.zeros_like(r)
    return (((y.double() - r).abs() - half) / (EPS24 * a).clamp_min(1e-300)).nan_to_num(nan=float("inf"))


def close(y, r, a, label="", slack=RGEMM_SLACK):
    """The bar for general inputs: |y - r| <= half_ulp_out(r) + slack * 2^-24 * A on every element.  Prints the worst excess in
    units of the slack; on failure the worst elements too."""
    ex = excess(y, r, a)
    worst = float(ex.max()) if ex.numel() else float("-inf")
    ok = bool((ex <= slack).all())
    print(f"router gemm {label} {str(y.dtype)[6:]}: worst excess {worst:.3f} x 2^-24 A = {worst / slack:.3f} x slack"
          + ("" if ok else f"  FAILED: {int((ex > slack).sum())}/{ex.numel()} elements over"))
    if not ok:
        for i in torch.topk(ex.reshape(-1), min(10, ex.numel())).indices.tolist():
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ex.shape))
            print(f"  {idx}: got {float(y.reshape(-1)[i]):.9g} statement {float(r.reshape(-1)[i]):.9g} A {float(a.reshape(-1)[i]):.6g} "
                  f"excess {float(ex.reshape(-1)[i]):.3f}")
    return ok


# ---- the kernels' order in float32 -----------------------------------------------------------------------------------------------
def fp32_model(x, wh, wl, scale, waves, splits, fp32_out=True):
    """The kernels' arithmetic on the CPU.  K is cut into 64-k steps; split s of `splits` takes steps
    [steps * s / splits, steps * (s + 1) / splits); inside a split the steps are dealt round-robin to `waves` accumulator pairs
    (4: the skinny kernels' waves; 1: the tile kernels).  An accumulator takes one 32-k matrix instruction at a time: the 32
    products summed exactly, added to the accumulator, rounded to fp32 once.  Each pair ends as fp32(acc_l * scale + acc_h), one
    rounding; four of them are summed (p0 + p1) + (p2 + p3); the splits' partials are added in split order."""
    m, k = x.shape
    n, steps = wh.shape[0], k // 64
    assert k % 64 == 0 and waves in (1, 4) and 1 <= splits <= steps
    s = float(torch.tensor(scale, dtype=torch.float32))
    xb = x.double().view(m, k // 32, 32)
    dh = torch.einsum("mbk,nbk->bmn", xb, wh.double().view(n, k // 32, 32))
    dl = torch.einsum("mbk,nbk->bmn", xb, wl.double().view(n, k // 32, 32))
    total = None
    for sp in range(splits):
        parts = []
        for w in range(waves):
            acc_h = torch.zeros(m, n, dtype=torch.float32)
            acc_l = torch.zeros(m, n, dtype=torch.float32)
            for c in range(steps * sp // splits + w, steps * (sp + 1) // splits, waves):
                for b in (2 * c, 2 * c + 1):
                    acc_h = (acc_h.double() + dh[b]).float()
                    acc_l = (acc_l.double() + dl[b]).float()
            parts.append((acc_l.double() * s + acc_h.double()).float())
        p = parts[0] if waves == 1 else (parts[0] + parts[1]) + (parts[2] + parts[3])
        total = p if total is None else total + p
    return total if fp32_out else total.bfloat16()


# ---- planted errors --------------------------------------------------------------------------------------------------------------
def _span(x, wh, wl, scale, k0, k1):
    return ref64(x[:, k0:k1].contiguous(), wh[:, k0:k1].contiguous(), wl[:, k0:k1].contiguous(), scale)[0]


PLANTED = ("low plane dropped", "low plane's last mantissa bit cleared", "scale doubled", "one 64-k step dropped",
           "one 64-k step doubled", "the neighbouring row's w_low", "planes swapped", "last split's partial left out")
"""Wrong kernels, as float64 results before the output rounding (planted()).  The truncating bf16 cast is the ninth:
bf16_truncated, applied to the right result."""


def planted(kind, x, wh, wl, scale):
    """The float64 result a kernel with the named defect would round; `scale doubled` is 1 / 128 used for 1 / 256, the dropped or
    doubled step is the one in the middle of k, the left-out partial the last of three."""
    k = x.shape[1]
    mid = (k // 64 // 2) * 64
    r = ref64(x, wh, wl, scale)[0]
    if kind == "low plane dropped":
        return ref64(x, wh, torch.zeros_like(wl), scale)[0]
    if kind == "low plane's last mantissa bit cleared":
        return ref64(x, wh, (wl.view(torch.int16) & -2).view(torch.bfloat16), scale)[0]
    if kind == "scale doubled":
        return ref64(x, wh, wl, 2 * scale)[0]
    if kind == "one 64-k step dropped":
        return r - _span(x, wh, wl, scale, mid, mid + 64)
    if kind == "one 64-k step doubled":
        return r + _span(x, wh, wl, scale, mid, mid + 64)
    if kind == "the neighbouring row's w_low":
        return ref64(x, wh, wl.roll(-1, 0), scale)[0]
    if kind == "planes swapped":
        return ref64(x, wl, wh, scale)[0]
    if kind == "last split's partial left out":
        return _span(x, wh, wl, scale, 0, (k // 64) * 2 // 3 * 64)
    raise ValueError(kind)
