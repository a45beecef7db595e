"""The statement of hpc.mla_rope_norm_store_kv in float64 PyTorch (CPU), constructed inputs, and the checks of its tests
(tests/test_mla_store_bar.py on the CPU, tests/test_mla_store.py on the GPU).  Both run the same check_outputs(): the CPU test
feeds it an fp32 model of a correct kernel and planted errors, the GPU test feeds it the kernel's outputs.

Statement.  Row r of kv_a is one new token of request b = the last one with q_index[b] <= r, at position
pos = num_seqlen_per_req[b] - (q_index[b + 1] - r); rows at or past q_index[-1] and rows with pos < 0 belong to no request.

    c         = kv_a[r, :512]
    lat[:512] = c / sqrt(mean(c^2) + eps) * kv_norm_weight
    lat[512:] = rot(kv_a[r, 512:576], cos_sin[pos])
    ckv_cache[block_ids[b, pos // P], pos % P, :576] = lat          and / or          out_ckv[r] = lat
    out_q_pe[r, h, :] = rot(q_pe[r, h, :], cos_sin[pos])

rot: (a, b) -> (a cos_i - b sin_i, b cos_i + a sin_i), cos_i = cos_sin[pos, i], sin_i = cos_sin[pos, 32 + i], i < 32; the pair is
elements (2i, 2i + 1) when interleaved, (i, i + 32) otherwise.  It is written out here on its own, not through oracle/rope.py's
helpers (only the cos / sin table is that module's, as the op's contract names it), so that an error cannot cancel.

Construction (seeded CPU generators):
* decode batches of mtp 0 / 1 / 3 whose new tokens sit, by the length's residue, on the last slots of a page, the first slots,
  across a page edge or inside a page; a prefill batch with uneven new-token counts, a request with no new token and a
  length-0 request; a request near position 160k;
* context lengths are offset by page-aligned bases, so that positions cover 0, a few hundred, 4096 and 8192+ in one batch;
* padding rows: the first half belongs to a trailing length-0 request (pos < 0), the rest lies past q_index[-1];
* the rows of every fifth request are multiplied by 1e-3 (the epsilon takes part in their norm), of another fifth by 30;
* only the pages that the op may write exist; every other block_ids entry names one guard page, which must come back
  byte-identical, as must a few pages of no request;
* kv_a is a slice of [rows, 2112], q_pe of [rows, H, 192], out_q_pe of a sentinel-filled [rows, H, 576]; the cache is
  contiguous, has a token stride of 640, or is a view into a larger pool."""
import functools
from types import SimpleNamespace

import torch

from oracle import rope as orc
from utils import ROPE_SLACK, rope_close, rope_excess

LAT, ROPE, DIM = 512, 64, 576
MAX_POS = 8768       # >= 8192 + 4 * 128 + 64, the longest constructed request of the page sizes used
FAR_POS = 163840     # the table of the far case: positions up to 163,836
BASES = (0, 256, 8192, 4096)  # context offsets: multiples of every page size
SENTINEL = -777.0
KV_A_AT, Q_PE_AT, Q_ABS_AT = 1536, 128, 512  # where the views start in their parents' last dims
LAYOUTS = ("plain", "padded", "pool")


@functools.lru_cache(maxsize=2)
def cos_sin_table(max_pos):
    return orc.generate_cos_sin_cache(max_pos, ROPE)


# ---------------------------------------------------------------------------------------------------- the statement
def row_positions(ns, q_index, rows):
    """(request, position) of every kv_a row, int64 [rows] each, -1 for rows of no request"""
    ns, qi = ns.long(), q_index.long()
    r = torch.arange(rows)
    req = ((qi[None, :-1] <= r[:, None]).sum(1) - 1).clamp_min(0)  # the last b with q_index[b] <= r
    pos = ns[req] - (qi[req + 1] - r)
    gone = (r >= qi[-1]) | (pos < 0)
    return req.masked_fill(gone, -1), pos.masked_fill(gone, -1)


def rotate64(t, cos, sin, interleaved):
    """rot of the module docstring on the last dim (64) of a float64 tensor; cos, sin broadcast against [..., 32]"""
    if interleaved:
        a, b = t[..., 0::2], t[..., 1::2]
        return torch.stack([a * cos - b * sin, b * cos + a * sin], -1).flatten(-2)
    a, b = t[..., :32], t[..., 32:]
    return torch.cat([a * cos - b * sin, b * cos + a * sin], -1)


def statement(kv_a, q_pe, cos_sin, weight, ns, q_index, interleaved, eps=1e-6):
    """(lat float64 [rows, 576], q float64 [rows, H, 64] or None, req, pos), unrounded; rows of no request are zero"""
    rows = kv_a.shape[0]
    req, pos = row_positions(ns, q_index, rows)
    x = kv_a.double()
    c = x[:, :LAT]
    lat = c / torch.sqrt((c * c).sum(-1, keepdim=True) / LAT + eps) * weight.double()
    cs = cos_sin[pos.clamp_min(0)].double()
    cos, sin = cs[:, :32], cs[:, 32:]
    live = (req >= 0).double()
    out = torch.cat([lat, rotate64(x[:, LAT:], cos, sin, interleaved)], -1) * live[:, None]
    q = None if q_pe is None else rotate64(q_pe.double(), cos[:, None], sin[:, None], interleaved) * live[:, None, None]
    return out, q, req, pos


# ------------------------------------------------------------------------------------------------------ the cases
def decode_requests(P, num_req, tpr):
    """tpr new tokens per request; by the length's residue mod P they are the last slots of a page (0), the first slots
    (tpr), straddle two pages (1, for tpr > 1), or sit inside one"""
    resid = (0, tpr, 1, P - 1, P // 2)
    return [(BASES[r % 4] + P + resid[r % 5], tpr) for r in range(num_req)]


def prefill_requests(P):
    """(total length, new tokens): uneven counts; a run over two page edges at 8192+, a whole one-token request, a whole
    request that ends on a page's last slot, one token on a first slot, 37 tokens at 4096+, a context with no new token, a
    length-0 request, a run from inside the first page on"""
    return [(8192 + 2 * P + 3, P + 5), (1, 1), (P, P), (256 + 2 * P + 1, 1), (4096 + 50, 37), (8192 + P // 2, 0), (0, 0),
            (3 * P + 7, 2 * P + 9)]


def far_requests(P):
    return [(FAR_POS - 3, 5), (FAR_POS - P, 2), (131072 + 1, 1)]


def build_case(name, reqs, H, P, seed, pad_rows=0, max_pos=MAX_POS):
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
    y = torch.zeros(rows, 2112)
    y[:real] = torch.randn(real, 2112, generator=g)
    q_src = torch.zeros(rows, H, 192)
    q_src[:real] = torch.randn(real, H, 192, generator=g)
    need = [(r, b) for r, (s, n) in enumerate(reqs) if n for b in range((s - n) // P, (s - 1) // P + 1)]
    nblocks = len(need) + 4
    perm = torch.randperm(nblocks, generator=g).int()
    guard = int(perm[0])
    bid = torch.full((len(ns), (max_pos + P - 1) // P), guard, dtype=torch.int32)
    for i, (r, b) in enumerate(need):
        bid[r, b] = perm[1 + i]
    return SimpleNamespace(
        name=name, reqs=reqs, num_req=num_req, H=H, P=P, rows=rows, real_rows=real, starts=starts, guard=guard, nblocks=nblocks,
        y=(y * scale[:, None]).bfloat16(), q_src=(q_src * scale[:, None, None]).bfloat16(),
        w=torch.randn(LAT, generator=g), cache0=torch.randn(nblocks, P, DIM, generator=g).bfloat16(),
        q_nope=torch.randn(rows, H, LAT, generator=g).bfloat16(), ns=torch.tensor(ns, dtype=torch.int32),
        q_index=torch.tensor(qi, dtype=torch.int32), bid=bid, cos_sin=cos_sin_table(max_pos), refs={})


CASES = ("decode_mtp0_7", "decode_mtp1_16", "decode_mtp3_7", "decode_mtp0_16", "prefill", "far")


@functools.lru_cache(maxsize=None)
def case(name, H, P):
    seed = 100 * CASES.index(name) + H + P
    if name.startswith("decode"):
        mtp, num_req = int(name[10]), int(name.split("_")[2])
        pad = (-num_req * (mtp + 1)) % 8  # to a multiple of 8 rows, and at least two padding rows: one of each kind
        return build_case(name, decode_requests(P, num_req, mtp + 1), H, P, seed, pad_rows=pad if pad >= 2 else pad + 8)
    if name == "prefill":
        return build_case(name, prefill_requests(P), H, P, seed, pad_rows=3)
    return build_case(name, far_requests(P), H, P, seed, max_pos=FAR_POS)


def reference(c, interleaved):
    """the float64 statement of the case, computed once per pairing and shared (read-only) by the tests"""
    if interleaved not in c.refs:
        lat, q, req, pos = statement(c.y[:, KV_A_AT: KV_A_AT + DIM], c.q_src[..., Q_PE_AT:], c.cos_sin, c.w, c.ns, c.q_index,
                                     interleaved)
        live = req >= 0
        idx = live.nonzero().squeeze(1)
        assert idx.numel() == c.real_rows
        page = c.bid[req[idx], pos[idx] // c.P].long()
        c.refs[interleaved] = SimpleNamespace(lat=lat, q=q, req=req, pos=pos, idx=idx, page=page, slot=pos[idx] % c.P)
    return c.refs[interleaved]


# ------------------------------------------------------------------------------------- buffers: stores and views
def spec(layout="plain", cache=True, out_ckv=False, q="abs"):
    """what a call is given: the cache layout (LAYOUTS), which destinations, and the q mode: None (no q_pe), "abs" (out_q_pe =
    q_abs[..., 512:]), "fresh" (no out_q_pe: the op allocates), "inplace" (out_q_pe is q_pe)"""
    assert layout in LAYOUTS and q in (None, "abs", "fresh", "inplace") and (cache or out_ckv)
    return SimpleNamespace(layout=layout, cache=cache, out_ckv=out_ckv, q=q)


def make_stores(c, sp):
    """the allocations of one call, on the CPU: every byte of them is compared with its value before the call, except the
    cells the op must write"""
    s = dict(y=c.y.clone(), q_src=c.q_src.clone(), w=c.w.clone(), ns=c.ns.clone(), q_index=c.q_index.clone(), bid=c.bid.clone())
    if sp.cache:
        shape = {"plain": (c.nblocks, c.P, DIM), "padded": (c.nblocks, c.P, 640), "pool": (c.nblocks + 2, c.P + 3, 640)}[sp.layout]
        s["cache"] = torch.full(shape, SENTINEL, dtype=torch.bfloat16)
    if sp.out_ckv:
        s["ockv"] = torch.full((c.rows, 640), SENTINEL, dtype=torch.bfloat16)
    if sp.q == "abs":
        s["q_abs"] = torch.full((c.rows, c.H, DIM), SENTINEL, dtype=torch.bfloat16)
        s["q_abs"][..., :Q_ABS_AT] = c.q_nope
    v = views(c, sp, s)
    if sp.cache:
        v.cache.copy_(c.cache0)
    return s


def views(c, sp, s):
    """the op's arguments as views of the stores `s` (CPU or GPU tensors, or the bool masks of check_outputs)"""
    v = SimpleNamespace(kv_a=s["y"][:, KV_A_AT: KV_A_AT + DIM], q_pe=None, out_q_pe=None, cache=None, out_ckv=None)
    if sp.q:
        v.q_pe = s["q_src"][..., Q_PE_AT:]
        v.out_q_pe = {"abs": lambda: s["q_abs"][..., Q_ABS_AT:], "inplace": lambda: v.q_pe, "fresh": lambda: None}[sp.q]()
    if sp.cache:
        t = s["cache"]
        v.cache = {"plain": t, "padded": t[:, :, :DIM], "pool": t[1:-1, 2: 2 + c.P, :DIM]}[sp.layout]
    if sp.out_ckv:
        v.out_ckv = s["ockv"][:, :DIM]
    return v


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def check_outputs(c, sp, after, before, ret, interleaved, slack=ROPE_SLACK, label=""):
    """Every check of one call, on CPU tensors.  after / before: the stores (make_stores) after and before the call; ret: what
    the op returned.  Returns the names of the checks that failed (empty: all hold); rope_close prints each output's worst
    excess over the half-ulp term.
      * the new tokens' cache rows, out_ckv and out_q_pe on the bar of utils.rope_close against the float64 statement: half a
        bf16 ulp plus ROPE_SLACK of the largest value of the row's 512 latent columns, of its k_pe, of the q head; rows of no
        request must be exactly zero in out_ckv and out_q_pe;
      * everything else byte for byte as before the call: the rest of the cache with its padding columns, guard pages and page
        tails, the padding of out_ckv, the columns :512 of the q buffer, the inputs (when not in place) and the tables."""
    ref = reference(c, interleaved)
    av = views(c, sp, after)
    failed = []

    def bar(name, want, got):
        if not rope_close(want, got, None, slack, f"{label} {name}"):
            failed.append(name)

    def bar_rows(name, want, got):  # [n, 576]: the latent columns and k_pe, each against its own largest value
        bar(name + " latent", want[:, None, :LAT], got[:, None, :LAT])
        bar(name + " k_pe", want[:, None, LAT:], got[:, None, LAT:])

    masks = {k: torch.zeros(t.shape, dtype=torch.bool) for k, t in after.items()}
    mv = views(c, sp, masks)
    if sp.cache:
        bar_rows("cache", ref.lat[ref.idx], av.cache[ref.page, ref.slot])
        mv.cache[ref.page, ref.slot] = True
    if sp.out_ckv:
        bar_rows("out_ckv", ref.lat, av.out_ckv)
        mv.out_ckv[:] = True
    if sp.q:
        if sp.q == "fresh":
            if ret is None or ret.shape != ref.q.shape or ret.dtype != torch.bfloat16 or not ret.is_contiguous():
                failed.append("returned q_pe")
            else:
                bar("q_pe", ref.q, ret)
        else:
            bar("q_pe", ref.q, av.out_q_pe)
            mv.out_q_pe[:] = True
    elif ret is not None:
        failed.append("returned something without q_pe")
    for k in after:
        if not torch.equal(_bits(after[k])[~masks[k]], _bits(before[k])[~masks[k]]):
            failed.append(f"{k} changed outside the written cells")
    if failed:
        print(f"check_outputs {label} FAILED: {failed}")
    return failed


def snapshot(stores):
    return {k: t.clone() for k, t in stores.items()}


# ---------------------------------------------------------------------- the fp32 model of a correct kernel, and mutants
def _rot32(t, cos, sin, interleaved):
    if interleaved:
        a, b = t[..., 0::2], t[..., 1::2]
        return torch.stack([a * cos - b * sin, b * cos + a * sin], -1).flatten(-2)
    a, b = t[..., :32], t[..., 32:]
    return torch.cat([a * cos - b * sin, b * cos + a * sin], -1)


def _truncate(t32):
    return (t32.view(torch.int32) & -65536).view(torch.float32).bfloat16()


def model(c, sp, stores, interleaved, eps=1e-6, mean_cols=LAT, on_kpe=None, normalise=True, sin_sign=1.0, pos_shift=0,
          other_pairing=False, neighbours_cos_sin=False, slot_shift=0, truncate=False, touch_q_nope=False, clear_tail=False):
    """The op in fp32 with one rounding, applied to the CPU stores; returns what the op returns.  The keywords plant errors
    (tests/test_mla_store_bar.py): another epsilon; the mean over 576 columns; the norm ("norm") or its weight ("weight") also
    on k_pe; no norm; the sine negated; positions off by one; the other pairing; the cos / sin of the neighbouring live row;
    the token stored one slot later; truncation; a write into the columns :512 of the q buffer; a cleared page tail."""
    v = views(c, sp, stores)
    req, pos = row_positions(stores["ns"], stores["q_index"], c.rows)
    live = req >= 0
    idx = live.nonzero().squeeze(1)
    x = v.kv_a.float()
    r = torch.rsqrt((x[:, :mean_cols] ** 2).sum(-1, keepdim=True) / mean_cols + torch.tensor(eps, dtype=torch.float32))
    lat = x[:, :LAT] * r * stores["w"] if normalise else x[:, :LAT]
    use = pos.clone()
    if neighbours_cos_sin:
        use[idx] = pos[idx.roll(1)]
    use = (use + pos_shift).clamp(0, c.cos_sin.shape[0] - 1)
    cs = c.cos_sin[use]
    cos, sin = cs[:, :32], cs[:, 32:] * sin_sign
    pairing = interleaved != other_pairing
    kpe = x[:, LAT:]
    if on_kpe == "norm":
        kpe = kpe * r
    elif on_kpe == "weight":
        kpe = kpe * stores["w"][:ROPE]
    rnd = _truncate if truncate else (lambda t: t.bfloat16())
    row = rnd(torch.cat([lat, _rot32(kpe, cos, sin, pairing)], -1).contiguous()) * live[:, None]
    if sp.cache:
        page = stores["bid"][req[idx], pos[idx] // c.P].long()
        slot = (pos[idx] + slot_shift) % c.P
        v.cache[page, slot] = row[idx]
        if clear_tail:
            ends = (pos[idx] == stores["ns"].long()[req[idx]] - 1) & (pos[idx] % c.P < c.P - 1)
            last = idx[ends][-1:]  # a request's last token that has a tail behind it
            v.cache[stores["bid"][req[last], pos[last] // c.P].long(), int(pos[last] % c.P) + 1:] = 0
    if sp.out_ckv:
        v.out_ckv.copy_(row)
    if not sp.q:
        return None
    q = rnd(_rot32(v.q_pe.float(), cos[:, None], sin[:, None], pairing).contiguous()) * live[:, None, None]
    if touch_q_nope and sp.q == "abs":
        stores["q_abs"][0, 0, Q_ABS_AT - 1] = 0
    if sp.q == "fresh":
        return q
    v.out_q_pe.copy_(q)
    return v.out_q_pe


def worst_excess(c, sp, after, ret, interleaved):
    """(latent, k_pe, q_pe) worst excess of a call's outputs over the half-ulp term: the figures ROPE_SLACK is a margin on"""
    ref, av = reference(c, interleaved), views(c, sp, after)
    got = av.cache[ref.page, ref.slot] if sp.cache else av.out_ckv[ref.idx]
    want = ref.lat[ref.idx]
    q = ret if sp.q == "fresh" else av.out_q_pe
    return (float(rope_excess(want[:, None, :LAT], got[:, None, :LAT]).max()),
            float(rope_excess(want[:, None, LAT:], got[:, None, LAT:]).max()),
            float(rope_excess(ref.q[ref.idx], q[ref.idx]).max()) if sp.q else 0.0)
