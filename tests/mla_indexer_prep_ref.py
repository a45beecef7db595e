"""The statement of hpc.mla_indexer_prep_fp8 in float64 PyTorch (CPU), written out on its own; the knobs the bar test turns to make
mutants; an fp32 model of the kernel's arithmetic in the kernel's butterfly and reduction order; the input constructions and
the check_outputs() the CPU test (tests/test_mla_indexer_prep.py, on the model and on planted errors) and the GPU test (on the
kernel's outputs) share; and the eager-torch chain a caller runs without the op.

Statement.  Row r is one new token of request b = the last one with q_index[b] <= r, at position
pos = num_seqlen_per_req[b] - (q_index[b + 1] - r); rows at or past q_index[-1] and rows with pos < 0 belong to no request.

    key      n = (x - mean(x)) / sqrt(var(x) + eps) * k_norm_weight + k_norm_bias, x = k[r], biased variance over the 128 columns
             n[:64] = rot(n[:64], cos_sin[pos]);   kr = H128(n) * rotate_scale                        (then ONE rounding to bf16)
    q head   x = q[r, h];  x[:64] = rot(x[:64], cos_sin[pos]);   qr = H128(x) * rotate_scale           (then ONE rounding to bf16)
    quant    on the bf16 rows: scale = amax / 448, code = e4m3(x * (1 / (scale + 1e-8)))   (tests/blockwise_quant_ref.py::quant), or
             with pow2_scale the smallest power of two >= amax / 448 and code = e4m3(x / scale)        (pow2_scale_of, quant_pow2)
    weights  fp32(fp32(head_weights * scale) * c), c = float32(softmax_scale * Hi ** -0.5)             (fold)

rot: (a, b) -> (a cos_i - b sin_i, b cos_i + a sin_i), cos_i = cos_sin[pos, i], sin_i = cos_sin[pos, 32 + i], i < 32; the pair is
columns (i, i + 32) (neox, interleaved False) or (2i, 2i + 1).  H128 is the explicit +-1 matrix H[i, j] = (-1)^popcount(i & j).
LayerNorm, rot and the pow2 rule are spelled out here, not taken from the op's helpers or from another test's reference, so
that an error cannot cancel; only the request constructions (which lengths land where in a page) are tests/mla_store_ref.py's."""
import functools
from types import SimpleNamespace

import torch

import mla_store_ref as ms
from utils import rope_excess

DIM, ROPE, TOKEN_BYTES = 128, 64, 132
F8 = torch.float8_e4m3fn
MAX_POS, FAR_POS = ms.MAX_POS, ms.FAR_POS
SENTINEL = -777.0
FILL = 0xA5
K_AT, K_WIDE, Q_PAD = 128, 384, 64  # k = parent[:, 128:256] of a [rows, 384] projection output; q rows padded by 64 elements

PREP_SLACK = 2.0 ** -21
"""fp32 slack of the front end's bar (check_outputs), as a fraction of the vector's largest |value| (utils.rope_excess).

Measured: model32 below - the kernel's arithmetic in fp32 in the kernel's order: lane sums of 8 then an xor tree for mean and
variance, torch.rsqrt, seven butterfly stages in natural order, one multiply by rotate_scale, one rounding - against the float64
statement on every case x configuration x pairing of tests/test_mla_indexer_prep.py has a worst excess of 4.27e-8 of the vector
maximum on the key (LayerNorm + RoPE + rotation) and 5.66e-8 on the queries (RoPE + rotation); test_bar_accepts_fp32_model
measures both again, prints them and holds the constant to them.  8 x 5.66e-8 = 4.53e-7, and the next power of two at or above
that is 2^-21 = 4.77e-7.  The margin is for what a correct kernel may do differently from the model: the hardware reciprocal
square root, fused multiply-adds in the affine step and in the rotation of the pairs.  Cap: 2^-16; a kernel that needs more is a
finding."""


# ---------------------------------------------------------------------------------------------------- the statement
@functools.lru_cache(maxsize=1)
def hadamard_matrix():
    """float64 [128, 128], H[i, j] = (-1)^popcount(i & j): the Sylvester-ordered Walsh-Hadamard matrix"""
    i = torch.arange(DIM)
    both = i[:, None] & i[None, :]
    pop = sum((both >> b) & 1 for b in range(7))
    return (1 - 2 * (pop & 1)).double()


def bit_reverse7(i):
    return sum(((i >> b) & 1) << (6 - b) for b in range(7))


def row_positions(ns, q_index, rows):
    """(request, position) of every row, int64 [rows] each, -1 for rows of no request"""
    ns, qi = ns.long(), q_index.long()
    req, pos = torch.full((rows,), -1, dtype=torch.int64), torch.full((rows,), -1, dtype=torch.int64)
    for r in range(rows):
        if r >= int(qi[-1]):
            continue
        b = max(i for i in range(len(ns)) if int(qi[i]) <= r)  # the last request with q_index[b] <= r
        p = int(ns[b]) - (int(qi[b + 1]) - r)
        if p >= 0:
            req[r], pos[r] = b, p
    return req, pos


def rot(t, cos, sin, interleaved):
    """rot of the module docstring on the last dim (64) of a float64 tensor; cos, sin broadcast against [..., 32]"""
    if interleaved:
        a, b = t[..., 0::2], t[..., 1::2]
        return torch.stack([a * cos - b * sin, b * cos + a * sin], -1).flatten(-2)
    a, b = t[..., :32], t[..., 32:]
    return torch.cat([a * cos - b * sin, b * cos + a * sin], -1)


def layer_norm(x, weight, bias, eps, *, subtract_mean=True, use_bias=True, unbiased=False):
    x = x.double()
    d = x - x.mean(-1, keepdim=True) if subtract_mean else x
    var = (d * d).sum(-1, keepdim=True) / (DIM - 1 if unbiased else DIM)
    n = d / torch.sqrt(var + eps) * weight.double()
    return n + bias.double() if use_bias else n


def statement(k, q, weight, bias, cos_sin, ns, q_index, *, interleaved=False, eps=1e-6, rotate_scale=DIM ** -0.5, rotate=True,
              rope_last=False, other_pairing=False, pos_shift=0, sin_sign=1.0, subtract_mean=True, use_bias=True, unbiased=False,
              use_rotate_scale=True, bit_reversed=False):
    """(kr float64 [T, 128], qr float64 [T, Hi, 128] or None, req, pos), unrounded; rows of no request are zero.  The keywords
    after rotate_scale are the mutations of test_bar_rejects_mutants, all off by default."""
    rows = k.shape[0]
    req, pos = row_positions(ns, q_index, rows)
    cs = cos_sin[(pos + pos_shift).clamp(0, cos_sin.shape[0] - 1)].double()
    cos, sin = cs[:, :32], cs[:, 32:] * sin_sign
    H = hadamard_matrix()
    if bit_reversed:
        H = H[bit_reverse7(torch.arange(DIM))]
    pairing = interleaved != other_pairing

    def front(t, cos, sin):
        if rope_last:
            t = torch.cat([t[..., :ROPE], rot(t[..., ROPE:], cos, sin, pairing)], -1)
        else:
            t = torch.cat([rot(t[..., :ROPE], cos, sin, pairing), t[..., ROPE:]], -1)
        if rotate:
            t = t @ H.T
        return t * rotate_scale if use_rotate_scale else t

    live = req >= 0
    n = layer_norm(k, weight, bias, eps, subtract_mean=subtract_mean, use_bias=use_bias, unbiased=unbiased)
    kr = front(n, cos, sin)
    kr = torch.where(live[:, None], kr, torch.zeros_like(kr))  # +0, not a product with 0: the op writes zero bits
    qr = None
    if q is not None:
        qr = front(q.double(), cos[:, None], sin[:, None])
        qr = torch.where(live[:, None, None], qr, torch.zeros_like(qr))
    return kr, qr, req, pos


def pow2_scale_of(amax):
    """the ue8m0 rule on float32 abs-maxima: of the bits of amax / 448 the exponent field goes up by one when the mantissa is
    non-zero and is clamped to [1, 254]; the mantissa is dropped"""
    bits = (amax.float() / 448.0).contiguous().view(torch.int32)
    e = ((bits >> 23) & 0xFF) + ((bits & 0x7FFFFF) != 0).int()
    return (e.clamp(1, 254) << 23).view(torch.float32)


def quant_pow2(a):
    """a [N, 128] -> (codes float8_e4m3fn [N, 128], scale float32 [N]) with the power-of-two scale; the division is exact"""
    x = a.float()
    scale = pow2_scale_of(x.abs().amax(-1))
    return (x / scale[:, None]).to(F8), scale


def fold(head_weights, scale, softmax_scale, Hi):
    """weights of the logits op: two float32 multiplies, each rounded"""
    c = torch.tensor(softmax_scale * Hi ** -0.5, dtype=torch.float32)
    return (head_weights.float() * scale.float()) * c


# ---------------------------------------------------------------------- the fp32 model of the kernel's arithmetic
def _sum16x8(x):
    """sum over the last dim (128) as the kernel forms it: each of 16 lanes adds its 8 columns in order, then an xor tree over
    the lanes at 1, 2, 4, 8"""
    lanes = x.reshape(x.shape[:-1] + (16, 8))
    s = lanes[..., 0]
    for i in range(1, 8):
        s = s + lanes[..., i]
    idx = torch.arange(16)
    for d in (1, 2, 4, 8):
        s = s + s[..., idx ^ d]
    return s[..., :1]


def _fwht32(t):
    """seven butterfly stages in natural order, stride 1 first: the lower index takes a + b, the upper a - b"""
    shape = t.shape
    h = 1
    while h < DIM:
        v = t.reshape(shape[:-1] + (DIM // (2 * h), 2, h))
        a, b = v[..., 0, :], v[..., 1, :]
        t = torch.stack([a + b, a - b], -2).reshape(shape)
        h *= 2
    return t


def model32(k, q, weight, bias, cos_sin, ns, q_index, *, interleaved=False, eps=1e-6, rotate_scale=DIM ** -0.5):
    """(out_k bf16 [T, 128], out_q_rot bf16 [T, Hi, 128] or None): the op in fp32 with one rounding, rows of no request zero"""
    rows = k.shape[0]
    req, pos = row_positions(ns, q_index, rows)
    cs = cos_sin[pos.clamp(0, cos_sin.shape[0] - 1)].float()
    cos, sin = cs[:, :32], cs[:, 32:]
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    x = k.float()
    d = x - _sum16x8(x) * f(1 / DIM)
    rstd = torch.rsqrt(_sum16x8(d * d) * f(1 / DIM) + f(eps))
    n = d * rstd * weight.float() + bias.float()

    def front(t, cos, sin):
        t = torch.cat([rot(t[..., :ROPE], cos, sin, interleaved), t[..., ROPE:]], -1)
        return (_fwht32(t.contiguous()) * f(rotate_scale)).bfloat16()

    live = req >= 0
    out_k = front(n, cos, sin)
    out_k = torch.where(live[:, None], out_k, torch.zeros_like(out_k))
    out_q = None
    if q is not None:
        out_q = front(q.float(), cos[:, None], sin[:, None])
        out_q = torch.where(live[:, None, None], out_q, torch.zeros_like(out_q))
    return out_k, out_q


# ------------------------------------------------------------------------------------------------------ the cases
CONFIGS = [(64, 64), (16, 16), (32, 128), (64, 32)]  # (Hi, P)
CASES = ("mix", "far")


def mix_requests(P):
    """decode batches of mtp 0 / 1 / 3 from tests/mla_store_ref.py (the new tokens on the last slots of a page, the first slots,
    across a page edge, inside a page), then a prefill batch: a run over a page edge at 8192+, a whole one-token request, one
    token on a first slot, 17 tokens at 256+, a context with no new token, a length-0 request, a run from inside the first page
    over its edge"""
    prefill = [(8192 + P + 3, 9), (1, 1), (4096 + 2 * P + 1, 1), (256 + 50, 17), (8192 + P // 2, 0), (0, 0), (P + 5, 11)]
    return ms.decode_requests(P, 5, 1) + ms.decode_requests(P, 5, 2) + ms.decode_requests(P, 5, 4) + prefill


def far_requests(P):
    return [(FAR_POS - 3, 5), (FAR_POS - P, 2), (131072 + 1, 1)]


@functools.lru_cache(maxsize=None)
def exact_cos_sin(max_pos):
    """a table whose entries are all in {0, +1, -1}: quarter turns, so that RoPE is exact in any float format"""
    g = torch.Generator().manual_seed(7)
    turn = torch.randint(0, 4, (max_pos, 32), generator=g)
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[turn]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[turn]
    return torch.cat([cos, sin], -1).contiguous()


def build_case(name, reqs, Hi, P, seed, *, pad_rows, max_pos, exact=False):
    """exact: q integer-valued in [-8, 8] and the quarter-turn table (use rotate_scale = 0.125): every intermediate of the
    query path is an integer below 2^24 or an eighth of one, and some outputs need rounding.  Otherwise bf16 Gaussian rows, those of every fifth request scaled
    by 1e-3 (eps takes part), of another fifth by 30, random norm weight and bias."""
    g = torch.Generator().manual_seed(seed)
    seq, new = [s for s, _ in reqs], [n for _, n in reqs]
    assert all(0 <= n <= s <= max_pos for s, n in reqs)
    num_req, real = len(reqs), sum(new)
    rows = real + pad_rows
    starts = [sum(new[:r]) for r in range(num_req + 1)]
    ns, qi = list(seq), list(starts)
    if pad_rows:  # a trailing length-0 request owns the first half of the padding rows; the rest lies past q_index[-1]
        ns.append(0)
        qi.append(real + pad_rows // 2)
    scale = torch.ones(rows)
    for r in range(num_req):
        scale[starts[r]: starts[r + 1]] = {1: 1e-3, 3: 30.0}.get(r % 5, 1.0)
    # padding rows hold data too: what comes back for them must be zeros whatever they hold
    k = torch.randn(rows, DIM, generator=g) * scale[:, None]
    if exact:
        q = torch.randint(-8, 9, (rows, Hi, DIM), generator=g).float()
        # eight heads whose unturned half follows a row of H with a few 7s among the 8s: outputs near 64 in eighths, which need
        # more than bf16's eight bits - the ONE rounding does round there, ties included
        for j in range(8):
            pattern = 8 * hadamard_matrix()[(37 * j + 5) % DIM, ROPE:].float()
            pattern[: j + 1] -= pattern[: j + 1].sign()
            q[j, j % Hi, ROPE:] = pattern
    else:
        q = torch.randn(rows, Hi, DIM, generator=g) * scale[:, None, None]
    need = [(r, b) for r, (s, n) in enumerate(reqs) if n for b in range((s - n) // P, (s - 1) // P + 1)]
    nblocks = len(need) + 4
    perm = torch.randperm(nblocks, generator=g).int()
    guard = int(perm[0])
    bid = torch.full((len(ns), (max_pos + P - 1) // P), guard, dtype=torch.int32)
    for i, (r, b) in enumerate(need):
        bid[r, b] = perm[1 + i]
    return SimpleNamespace(
        name=name, reqs=reqs, num_req=num_req, Hi=Hi, P=P, rows=rows, real_rows=real, starts=starts, guard=guard, nblocks=nblocks,
        exact=exact, k=k.bfloat16(), q=q.bfloat16(), w=torch.randn(DIM, generator=g), b=0.5 * torch.randn(DIM, generator=g),
        head_weights=torch.randn(rows, Hi, generator=g), ns=torch.tensor(ns, dtype=torch.int32),
        q_index=torch.tensor(qi, dtype=torch.int32), bid=bid, softmax_scale=DIM ** -0.5,
        cos_sin=exact_cos_sin(max_pos) if exact else ms.cos_sin_table(max_pos), refs={})


@functools.lru_cache(maxsize=None)
def case(name, Hi, P, exact=False):
    seed = 1000 * CASES.index(name) + 10 * Hi + P + (5 if exact else 0)
    if name == "mix":
        return build_case(name, mix_requests(P), Hi, P, seed, pad_rows=3, max_pos=MAX_POS, exact=exact)
    return build_case(name, far_requests(P), Hi, P, seed, pad_rows=2, max_pos=FAR_POS, exact=exact)


def reference(c, interleaved, rotate_scale=DIM ** -0.5):
    """the float64 statement of the case, computed once per (pairing, rotate_scale) and shared (read-only) by the tests"""
    key = (interleaved, rotate_scale)
    if key not in c.refs:
        kr, qr, req, pos = statement(c.k, c.q, c.w, c.b, c.cos_sin, c.ns, c.q_index, interleaved=interleaved, rotate_scale=rotate_scale)
        idx = (req >= 0).nonzero().squeeze(1)
        assert idx.numel() == c.real_rows
        page = c.bid[req[idx], pos[idx] // c.P].long()
        c.refs[key] = SimpleNamespace(k=kr, q=qr, req=req, pos=pos, idx=idx, dead=(req < 0).nonzero().squeeze(1), page=page,
                                      slot=pos[idx] % c.P)
    return c.refs[key]


def parents(c, device="cpu"):
    """k as a slice of a wider projection output and q with a padded row stride, both inside sentinel-filled parents; returns
    (k parent, q parent, k view, q view)"""
    kp = torch.full((c.rows, K_WIDE), SENTINEL, dtype=torch.bfloat16)
    kp[:, K_AT: K_AT + DIM] = c.k
    qp = torch.full((c.rows, c.Hi * DIM + Q_PAD), SENTINEL, dtype=torch.bfloat16)
    qp[:, : c.Hi * DIM] = c.q.reshape(c.rows, c.Hi * DIM)
    kp, qp = kp.to(device), qp.to(device)
    return kp, qp, kp[:, K_AT: K_AT + DIM], qp[:, : c.Hi * DIM].unflatten(1, (c.Hi, DIM))


def expected_cache(c, ref, codes, scales, cache0):
    """cache0 (uint8 [nblocks, P * 132]) with the codes (float8 [T, 128]) and scales (float32 [T]) of the live rows in their
    cells and every other byte as it was"""
    want = cache0.clone()
    P = c.P
    for i, r in enumerate(ref.idx.tolist()):
        page, t = int(ref.page[i]), int(ref.slot[i])
        want[page, DIM * t: DIM * t + DIM] = codes[r].view(torch.uint8)
        want[page, DIM * P + 4 * t: DIM * P + 4 * t + 4] = scales[r: r + 1].view(torch.uint8)
    return want


# ------------------------------------------------------------------------------------------------------ the checks
def worst_excess(c, interleaved, out_k, out_q_rot, rotate_scale=DIM ** -0.5):
    """(key, queries) worst excess of a call's bf16 outputs over the half-ulp term, as a fraction of the vector's largest |value|:
    the figures PREP_SLACK is a margin on"""
    ref = reference(c, interleaved, rotate_scale)
    return (float(rope_excess(ref.k[ref.idx][:, None], out_k[ref.idx][:, None]).max()),
            float(rope_excess(ref.q[ref.idx], out_q_rot[ref.idx]).max()) if out_q_rot is not None else 0.0)


def check_outputs(c, interleaved, out_k, out_q_rot, slack=PREP_SLACK, label="", rotate_scale=DIM ** -0.5):
    """Every check of the bf16 outputs of one call, on CPU tensors; returns the names of the checks that failed (empty: all hold)
    and prints each output's worst excess in units of the slack.
      * every vector of out_k / out_q_rot of a row of a request within half a bf16 ulp of the float64 statement plus `slack` x
        the vector's largest |value| (utils.rope_excess);
      * rows of no request exactly zero."""
    ref = reference(c, interleaved, rotate_scale)
    failed = []
    for name, want, got in (("out_k", ref.k[:, None], None if out_k is None else out_k[:, None]), ("out_q_rot", ref.q, out_q_rot)):
        if got is None:
            continue
        if got.shape != want.shape or got.dtype != torch.bfloat16:
            failed.append(name + " shape or dtype")
            continue
        ex = rope_excess(want[ref.idx], got[ref.idx])
        worst = float(ex.max())
        print(f"check_outputs {label} {name}: worst excess {worst:.3g} of the vector maximum = {worst / slack:.3g} x slack")
        if not bool((ex <= slack).all()):
            failed.append(name)
        if ref.dead.numel() and not bool((got[ref.dead].float() == 0).all()):
            failed.append(name + " rows of no request")
    if failed:
        print(f"check_outputs {label} FAILED: {failed}")
    return failed


# the mutants of plausible bugs the bar must reject (keywords of statement())
MUTANTS = {
    "rotation left out": dict(rotate=False),
    "RoPE on the last 64 columns": dict(rope_last=True),
    "interleaved taken for neox": dict(other_pairing=True),
    "position off by one": dict(pos_shift=1),
    "sin sign flipped": dict(sin_sign=-1.0),
    "mean not subtracted (RMSNorm)": dict(subtract_mean=False),
    "bias dropped": dict(use_bias=False),
    "variance unbiased (/ 127)": dict(unbiased=True),
    "another eps (1e-5)": dict(eps=1e-5),
    "rotate_scale left out": dict(use_rotate_scale=False),
    "Hadamard rows in bit-reversed order": dict(bit_reversed=True),
}
KEY_ONLY = {"mean not subtracted (RMSNorm)", "bias dropped", "variance unbiased (/ 127)", "another eps (1e-5)"}


# ---- what a caller runs without the op -----------------------------------------------------------------------------------------
def prep_eager(k_cache, k, weight, bias, cos_sin, ns, q_index, block_ids, q, head_weights, softmax_scale, *, eps=1e-6,
               rotate_scale=DIM ** -0.5, hadamard=None):
    """The chain in eager torch on k's device (neox pairing): LayerNorm, RoPE, a matmul by the Hadamard matrix,
    hpc.blockwise_fp8_quant, the fold, hpc.mla_indexer_store_k_fp8.  ns / q_index as int tensors on the device: the positions
    are formed there, nothing is read by the host.  hadamard: the float32 matrix on k's device (made here when not given: a
    copy from the host).  Returns (q8, weights)."""
    import hpc

    rows, Hi = q.shape[0], q.shape[1]
    r = torch.arange(rows, device=k.device)
    req = (torch.searchsorted(q_index[1:].long().contiguous(), r, right=True)).clamp_max(ns.shape[0] - 1)
    pos = (ns.long()[req] - (q_index.long()[req + 1] - r)).clamp(0, cos_sin.shape[0] - 1)
    cs = cos_sin[pos]
    cos, sin = cs[:, None, :32], cs[:, None, 32:]
    H = hadamard if hadamard is not None else hadamard_matrix().to(device=k.device, dtype=torch.float32)

    def front(t):
        a, b = t[..., :32], t[..., 32:ROPE]
        t = torch.cat([a * cos - b * sin, b * cos + a * sin, t[..., ROPE:]], -1)
        return ((t @ H) * rotate_scale).bfloat16()

    n = torch.nn.functional.layer_norm(k.float(), (DIM,), weight, bias, eps)
    kr = front(n[:, None])[:, 0].contiguous()
    qr = front(q.float())
    q8, qs = hpc.blockwise_fp8_quant(qr.reshape(rows * Hi, DIM))
    weights = head_weights.float() * qs.view(rows, Hi) * (softmax_scale * Hi ** -0.5)
    hpc.mla_indexer_store_k_fp8(k_cache, kr, ns, q_index, block_ids)
    return q8.view(rows, Hi, DIM), weights
