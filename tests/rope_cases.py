"""Constructed inputs, the cache expectation and the checks of the rope + KV store tests (tests/test_rope_bar.py on the
CPU, tests/test_rope_exact.py on the GPU).  Both run the same check_outputs(): the CPU test feeds it the fp32 oracle's
outputs and planted errors, the GPU test feeds it the kernel's.

Construction (seeded CPU generators, nothing drawn that matters):
* request lengths are constructed so that every page edge occurs: last token in the last slot of its page (no tail to
  clear), in the first slot, runs of new tokens that cross a page boundary, a request with no new token;
* context lengths are offset by page-aligned bases, so that absolute positions cover 0, a few hundred, 4096 and 8192+
  within one batch (the high neox pairs only turn visibly at large positions);
* only the pages that the op may write exist; every other kvcache_indices entry names one guard page, which must come
  back byte-identical, as must a few pages of no request;
* the rows of every 16th request are multiplied by 1e-3, so that the RMSNorm epsilon takes part in their norm."""
import functools
from types import SimpleNamespace

import torch

from oracle import rope as orc
from utils import ROPE_SLACK, rope_close, rope_excess

F8 = torch.float8_e4m3fn
D = 128
MAX_POS = 8768  # >= 8192 + 2 * 256 + 1, the longest constructed request
BASES = (0, 256, 8192, 4096)  # context offsets: multiples of every block size used (16, 64, 256)
SMALL_EVERY, SMALL_AT, SMALL = 16, 1, 1e-3  # requests r with r % 16 == 1 get rows of scale 1e-3


def is_wide(num_rows, heads_total):
    """Restates the rule of launch_rope in hpc-ops_amd/csrc/rope.hip: two groups of eight heads per wave
    (rope_kernel<*, 2>) from 16384 (row, group) units on, when a row has more than one group.  num_rows counts the
    padding rows of qkv too."""
    octs = (heads_total + 7) // 8
    return num_rows * octs >= 16384 and octs >= 2


@functools.lru_cache(maxsize=1)
def cos_sin_table():
    return orc.generate_cos_sin_cache(MAX_POS, D)


def prefill_requests(P):
    """(seqlen, new tokens) per request: total lengths 1, P-1, P, P+1, 2P, 2P+1 past a page-aligned context offset, each
    with one new token, with the whole request new (offset 0), and with a run of new tokens that starts in the slot
    before the last token's page (crosses a page boundary); and one request with a context and no new token."""
    reqs = []
    for i, L in enumerate((1, P - 1, P, P + 1, 2 * P, 2 * P + 1)):
        reqs.append((BASES[i % 4] + L, 1))
        reqs.append((L, L))
        reqs.append((BASES[1 + i % 3] + L, (L - 1) % P + 2))
    reqs.insert(8, (BASES[2] + P // 2, 0))
    return reqs


def decode_requests(P, num_req, tpr):
    """tpr new tokens per request; by the length's residue mod P they are the last slots of a page (0), the first slots
    (tpr), straddle two pages (1, for tpr > 1), or sit inside one."""
    resid = (0, tpr, 1, P - 1, P // 2)
    return [(BASES[r % 4] + P + resid[r % 5], tpr) for r in range(num_req)]


def uneven_requests(rows):
    """six prefill requests that share `rows` new tokens unevenly; contexts put positions at 0 ... 8192+"""
    q = [1, 37, rows // 11, rows // 4, rows // 3]
    q.append(rows - sum(q))
    ctx = [8192, 0, 256, 8000 - q[3], 0, MAX_POS - q[5] - 7]
    return [(c + n, n) for c, n in zip(ctx, q)]


def build_case(reqs, hq, hkv, P, seed, pad8=False, interleaved=False, extra_pages=3):
    g = torch.Generator().manual_seed(seed)
    num_req, ht = len(reqs), hq + 2 * hkv
    seq, ql = [s for s, _ in reqs], [n for _, n in reqs]
    assert all(0 <= n <= s <= MAX_POS for s, n in reqs)
    real_rows = sum(ql)
    rows = (real_rows + 7) // 8 * 8 if pad8 else real_rows
    nreq_p = (num_req + 7) // 8 * 8 if pad8 else num_req
    x = torch.zeros(rows, ht * D)
    x[:real_rows] = torch.randn(real_rows, ht * D, generator=g)
    starts = [sum(ql[:r]) for r in range(num_req + 1)]
    small = [r for r in range(num_req) if r % SMALL_EVERY == SMALL_AT]
    for r in small:
        x[starts[r] : starts[r + 1]] *= SMALL
    q_index = torch.full((nreq_p + 1,), rows, dtype=torch.int32)
    q_index[: num_req + 1] = torch.tensor(starts, dtype=torch.int32)
    ns = torch.zeros(nreq_p, dtype=torch.int32)
    ns[:num_req] = torch.tensor(seq, dtype=torch.int32)
    # pages the op may write: those of the new tokens, and the last page of every request with a context (its tail)
    need = []
    for r, (s, n) in enumerate(reqs):
        if s > 0:
            need += [(r, b) for b in range((s - n) // P if n else (s - 1) // P, (s - 1) // P + 1)]
    nblocks = len(need) + extra_pages + 1
    perm = torch.randperm(nblocks, generator=g).int()
    guard = int(perm[0])
    ki = torch.full((nreq_p, (MAX_POS + P - 1) // P), guard, dtype=torch.int32)
    for i, (r, b) in enumerate(need):
        ki[r, b] = perm[1 + i]
    if interleaved:  # K and V are the two halves of one allocation: block stride 2 * P * Hkv * 128
        buf = torch.randn(nblocks, 2, P, hkv, D, generator=g).bfloat16()
    else:
        buf = None
    kc = buf[:, 0] if interleaved else torch.randn(nblocks, P, hkv, D, generator=g).bfloat16()
    vc = buf[:, 1] if interleaved else torch.randn(nblocks, P, hkv, D, generator=g).bfloat16()
    return SimpleNamespace(
        reqs=reqs, num_req=num_req, hq=hq, hkv=hkv, P=P, rows=rows, real_rows=real_rows, small=small, starts=starts,
        qkv=x.bfloat16(), ns=ns, q_index=q_index, ki=ki, guard=guard, nblocks=nblocks, buf=buf, kc=kc, vc=vc,
        qw=torch.randn(D, generator=g), kw=torch.randn(D, generator=g), cos_sin=cos_sin_table(), refs={},
        max_new=max(ql))


@functools.lru_cache(maxsize=2)
def prefill_case(hq, hkv, P, interleaved=False):
    return build_case(prefill_requests(P), hq, hkv, P, seed=1000 + 10 * hq + P, interleaved=interleaved)


@functools.lru_cache(maxsize=2)
def decode_case(hq, hkv, P, num_req, mtp, interleaved=False):
    return build_case(decode_requests(P, num_req, mtp + 1), hq, hkv, P, seed=2000 + 10 * hq + P + num_req + mtp, pad8=True,
                      interleaved=interleaved)


@functools.lru_cache(maxsize=1)
def wide_prefill_case(hq, hkv, rows):
    return build_case(uneven_requests(rows), hq, hkv, 64, seed=3000 + hq)


@functools.lru_cache(maxsize=1)
def wide_decode_case(hq, hkv, num_req, mtp, P):
    return build_case(decode_requests(P, num_req, mtp + 1), hq, hkv, P, seed=4000 + hq, pad8=True)


def fresh_caches(case, fp8, device="cpu"):
    """(kcache, vcache) as the op gets them: copies, e4m3 for fp8, the two halves of one allocation if the case is
    interleaved."""
    def copy(t):
        return (t.to(F8) if fp8 else t.clone()).to(device)

    if case.buf is not None:
        b = copy(case.buf)
        return b[:, 0], b[:, 1]
    return copy(case.kc), copy(case.vc)


def reference(case, policy):
    """The float64 statement for the case, computed once per norm policy and shared (read-only) by the tests."""
    if policy not in case.refs:
        c = case
        q64, k64, req, pos = orc.rope_norm_ref64(c.kc, c.vc, c.qkv, c.cos_sin, c.ns, c.q_index, c.ki, c.qw, c.kw, policy)
        v = c.qkv[:, (c.hq + c.hkv) * D :].view(c.rows, c.hkv, D)
        case.refs[policy] = SimpleNamespace(q64=q64, k64=k64, v=v, req=req, pos=pos)
    return case.refs[policy]


def cache_expectation(case, req, pos):
    """Where the op writes: per qkv row the physical page and slot of its K / V (-1 for rows of no request), and
    tail [blocks, P] bool, the slots it zeroes.  The rule is the kernel's and the reference kernel's ("clear blocks"),
    not rope_norm_ref's: the tail of a request's last page is zeroed whenever seqlen > 0, even when the request has no
    new token in this call."""
    P = case.P
    live = req >= 0
    page = torch.where(live, case.ki[req.clamp_min(0), pos.clamp_min(0) // P].long(), torch.full_like(req, -1))
    slot = torch.where(live, pos % P, torch.full_like(pos, -1))
    tail = torch.zeros(case.nblocks, P, dtype=torch.bool)
    for r, (s, _) in enumerate(case.reqs):
        if s > 0:
            tail[int(case.ki[r, (s - 1) // P]), (s - 1) % P + 1 :] = True
    return page, slot, tail


def close_to_ref64(q, kcache, kcache0, qkv, cos_sin, ns, q_index, ki, qw, kw, policy, out_k=None, label=""):
    """The bar of utils.rope_close for a bf16 call on plain inputs (the earlier tests' generators, the golden fixtures),
    all on the CPU: Q of every row of a request, and K at the new tokens' cells of `kcache` (or in out_k)."""
    q64, k64, req, pos = orc.rope_norm_ref64(kcache0, kcache0, qkv, cos_sin, ns, q_index, ki, qw, kw, policy)
    idx = (req >= 0).nonzero().squeeze(1)
    P = kcache0.shape[1]
    k = out_k[idx] if out_k is not None else kcache[ki[req[idx], pos[idx] // P].long(), pos[idx] % P]
    return rope_close(q64[idx], q[idx], label=label + " Q") & rope_close(k64[idx], k, label=label + " K")


def fp32_rows(case, policy, eps=None, qw=None, kw=None, cos_sin=None, pos=None):
    """The fp32 oracle's arithmetic (oracle/rope.py rms_norm / rotary_neox in fp32) per qkv row, before the one rounding:
    q32 [rows, Hq, 128], k32 [rows, Hkv, 128].  The keywords plant errors (tests/test_rope_bar.py)."""
    c = case
    qw, kw = c.qw if qw is None else qw, c.kw if kw is None else kw
    pos = orc.rope_rows(c.ns, c.q_index, c.rows)[1] if pos is None else pos
    cs = (c.cos_sin if cos_sin is None else cos_sin)[pos.clamp_min(0)]
    q = c.qkv[:, : c.hq * D].float().view(c.rows, c.hq, D)
    k = c.qkv[:, c.hq * D : (c.hq + c.hkv) * D].float().view(c.rows, c.hkv, D)
    e = {} if eps is None else {"eps": eps}  # the oracle's own epsilon unless one is planted
    if policy == 2:
        q, k = orc.rms_norm(q, qw, **e), orc.rms_norm(k, kw, **e)
    q, k = orc.rotary_neox(q, cs), orc.rotary_neox(k, cs)
    if policy == 1:
        q, k = orc.rms_norm(q, qw, **e), orc.rms_norm(k, kw, **e)
    return q, k


def to_e4m3(x32, mult, saturate=True):
    y = x32 * mult
    return (y.clamp(-448.0, 448.0) if saturate else y).to(F8)


def emulate(case, policy, fp8, quant_policy=None, k_scale=None, v_scale=None, q_scale_inv=None, upper_max=448.0,
            bypass=False, is_prefill=True, rows32=None, saturate=True):
    """What the op returns and leaves in the caches, from the fp32 oracle's arithmetic (fp32_rows, or `rows32` with a
    planted error) rounded once, written by cache_expectation's rule: the `out` of check_outputs."""
    c = case
    q32, k32 = fp32_rows(c, policy) if rows32 is None else rows32
    req, pos = orc.rope_rows(c.ns, c.q_index, c.rows)
    page, slot, tail = cache_expectation(c, req, pos)
    idx = (req >= 0).nonzero().squeeze(1)
    v32 = c.qkv[:, (c.hq + c.hkv) * D :].float().view(c.rows, c.hkv, D)
    kc, vc = fresh_caches(c, fp8)
    out = SimpleNamespace(kc=kc, vc=vc, q_scale=None, out_k=None, out_v=None, flag=None)
    one = torch.ones((), dtype=torch.float32)
    if fp8:
        out.flag = torch.zeros(c.ns.shape[0], c.hkv, dtype=torch.int32)
        if quant_policy == 1:
            sc = q32.abs().amax(-1) / torch.tensor(upper_max, dtype=torch.float32)
            out.q = to_e4m3(q32, (one / sc).unsqueeze(-1))
            if is_prefill:
                pad = (c.max_new + 127) // 128 * 128
                out.q_scale = torch.full((c.ns.shape[0], c.hq, pad), float("nan"))
                out.q_scale[req[idx], :, idx - c.q_index.long()[req[idx]]] = sc[idx]
            else:
                out.q_scale = sc
        else:
            out.q = to_e4m3(q32, q_scale_inv)
        k, v = to_e4m3(k32, one / k_scale, saturate), to_e4m3(v32, one / v_scale, saturate)
    else:
        out.q, k, v = q32.bfloat16(), k32.bfloat16(), v32.bfloat16()
    if bypass:
        out.out_k, out.out_v = k, v
    else:
        for cache, new in ((kc, k), (vc, v)):  # through byte views: e4m3 tensors take no indexed assignment
            _bytes(cache)[page[idx], slot[idx]] = _bytes(new[idx])
            _bytes(cache)[tail] = 0
    return out


def _bytes(t):
    return t.view(torch.uint8 if t.element_size() == 1 else torch.int16)


def check_outputs(case, policy, out, before, fp8, quant_policy=None, k_scale=None, v_scale=None, q_scale_inv=None,
                  upper_max=448.0, bypass=False, is_prefill=True, slack=ROPE_SLACK, label=""):
    """Every check of one call, on CPU tensors.  `out`: q, kc, vc (caches after the call), q_scale, flag, out_k, out_v;
    `before`: the caches as they were.  Returns the names of the checks that failed (empty: all hold) and prints each
    output's worst excess over the half-ulp term.
      * Q, and K at the new tokens' cells (or in out_k), on the bar of utils.rope_close against the float64 statement;
      * V a pure copy: bit-equal in bf16, on the e4m3 bar in fp8;
      * dynamic q_scale = amax_d |q64| / upper_max within 2^-20 relative, and the largest |code| of a head = upper_max;
      * cleared tails all-zero bytes; every other byte of both caches as before the call; split_k_flag zero."""
    c, ref = case, reference(case, policy)
    page, slot, tail = cache_expectation(c, ref.req, ref.pos)
    idx = (ref.req >= 0).nonzero().squeeze(1)
    assert idx.numel() == c.real_rows
    q64, k64, v64 = ref.q64[idx], ref.k64[idx], ref.v[idx].double()
    one = torch.ones((), dtype=torch.float32)
    failed = []

    def bar(name, r64, got, mult=None):
        if not rope_close(r64, got, mult, slack, f"{label} {name}"):
            failed.append(name)

    if not fp8:
        bar("Q", q64, out.q[idx])
    elif quant_policy == 1:
        rq = ref.req[idx]
        qs = out.q_scale[rq, :, idx - c.q_index.long()[rq]] if is_prefill else out.q_scale[idx]
        want = q64.abs().amax(-1) / upper_max
        rel = float(((qs.double() - want).abs() / want).nan_to_num(nan=float("inf")).max())
        print(f"rope q_scale {label}: worst relative error {rel:.3g} = {rel * 2 ** 20:.3g} x 2^-20")
        if not rel <= 2.0 ** -20:
            failed.append("q_scale")
        if not bool((out.q[idx].float().abs().amax(-1) == upper_max).all()):
            failed.append("largest |code| == upper_max")
        bar("Q", q64, out.q[idx], one / qs)
    else:
        bar("Q", q64, out.q[idx], q_scale_inv)
    km, vm = (one / k_scale, one / v_scale) if fp8 else (None, None)
    if bypass:
        gk, gv = out.out_k[idx], out.out_v[idx]
        touched = torch.zeros(c.nblocks, c.P, dtype=torch.bool)
    else:
        gk, gv = out.kc[page[idx], slot[idx]], out.vc[page[idx], slot[idx]]
        touched = tail.clone()
        touched[page[idx], slot[idx]] = True
        for name, cache in (("K tail", out.kc), ("V tail", out.vc)):
            if int(_bytes(cache[tail]).ne(0).sum()):
                failed.append(name + " not zero")
    bar("K", k64, gk, km)
    if fp8:
        bar("V", v64, gv, vm)
    elif not torch.equal(_bytes(gv), _bytes(ref.v[idx])):
        failed.append("V not a copy")
    for name, cache, was in (("K", out.kc, before[0]), ("V", out.vc, before[1])):
        if not torch.equal(_bytes(cache[~touched]), _bytes(was[~touched])):
            failed.append(name + " cache changed outside the written cells")
    if fp8 and int(out.flag[: c.num_req].ne(0).sum()):
        failed.append("split_k_flag")
    if failed:
        print(f"check_outputs {label} FAILED: {failed}")
    return failed


def worst_excess(case, policy, out, fp8, mult_q=None, mult_kv=None):
    """(Q, K) worst excess of emulate()'s static outputs: the figure ROPE_SLACK is a margin on"""
    ref = reference(case, policy)
    page, slot, _ = cache_expectation(case, ref.req, ref.pos)
    idx = (ref.req >= 0).nonzero().squeeze(1)
    return (float(rope_excess(ref.q64[idx], out.q[idx], mult_q).max()),
            float(rope_excess(ref.k64[idx], out.kc[page[idx], slot[idx]], mult_kv).max()))
