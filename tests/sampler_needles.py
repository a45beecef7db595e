"""Planted-noise probes of hpc.fused_sampler - generator, CPU only (used by test_sampler_bar.py and
test_sampler_needles.py).

fused_sampler returns one token per row.  With gumbel_noise zero everywhere except one chosen token, that token answers
one yes/no question about what the kernels computed for the row: which candidates survive top-k and top-p, which score a
candidate carries after penalty, temperature and softmax, where the top-p cut falls.  A batch of rows is a batch of
questions and one call answers them all.

Logits row (plant_row): max_topk + 4 tokens on a descending ladder over a background, every value bf16-exact so that
fp32 and bf16 logits carry the same numbers.  Planted positions include token 0, token V - 1 and both sides of segment
boundaries of the top-k path (segments(), restated from hpc_sampler_segments and the launcher's rounding).  Four rank
pairs hold equal values, the smaller token id ranking first: (5, 6) inside the top-k, (19, 20) across the topk = 20
cut, (max_topk - 1, max_topk) across that cut and (max_topk + 2, max_topk + 3) beyond it.
  family A: ladder 4 - 0.25 r (crosses zero: both penalty branches) over a background near -30.
  family B: ladder 6 - 0.125 r over a background near -4, which carries a share of the full-vocabulary softmax mass
            that grows with V (policy 1's normaliser and its merge over segments).

Probes, all built from State: the stable descending order of the processed scores (penalty, then temperature, in fp32
as the oracle does) and the float64 log-scores g, probabilities p and exclusive cumulative probabilities c of its ranks.
  member  +1000 at the rank-r token, r = 0 .. max_topk + 1: the answer is that token iff rank r is kept, else rank 0's.
  score   for every kept rank i >= 1 two rows, noise g0 - gi + M and g0 - gi - M at the rank-i token: rank i wins the
          first, rank 0 the second.
  topp    for every rank r = 1 .. topk - 1 two rows, +1000 at the rank-r token, per-row topp c_r (1 + M) and
          c_r (1 - M): rank r wins the first, rank 0 the second.
  sweep   per-row topk = 1 .. max_topk (int32 or int64), +1000 at rank topk - 1 and at rank topk.
  token   +1000 at a named token (write-back case).

M = 1e-3 is a condition on the INPUTS, not a tolerance on the kernel: every decision a probe row asks for (a score
difference, a cumulative probability against topp) is at least M away from its threshold in float64, so the fp32 oracle
alone lands on the intended side.  Measured by test_sampler_bar.py::test_probes_are_the_oracles_answers over every case
of all_cases(): largest |fp32 g - float64 g| = 1.29e-6, largest |fp32 c_r - float64 c_r| / c_r = 1.09e-6 - M is 775 x
the larger (the test asserts 16 x).  With a penalty every row has its own mask row; a row whose decision would fall within M of a threshold gets
its mask row redrawn (the inputs are chosen, the bar is not moved).
"""
import functools
import math

import torch

from oracle import sampler as orc

M = 1e-3
BIG = 1000.0

# (policy, topk, topp, temperature, repetition penalty): the configurations of the probe batches
CONFIGS = (
    dict(policy=0, topk=20, topp=0.0, T=0.0, rp=0.0),
    dict(policy=0, topk=0, topp=0.0, T=0.0, rp=0.0),
    dict(policy=2, topk=20, topp=0.9, T=0.0, rp=0.0),
    dict(policy=1, topk=20, topp=0.9, T=0.0, rp=0.0),
    dict(policy=2, topk=20, topp=0.6, T=0.5, rp=0.0),
    dict(policy=2, topk=20, topp=0.9, T=0.5, rp=1.25),
    dict(policy=0, topk=20, topp=0.0, T=2.0, rp=2.0),
)
SMALL_V = (24, 264, 1024, 8200)
MAX_TOPK = (32, 64)


def segments(V):
    """(S, seg) of the top-k path: S workgroups per row, each owning seg consecutive tokens (the last ones may be
    ragged or empty)."""
    S = max(16, -(-V // 8192))
    return S, -(-(-(-V // S)) // 256) * 256


def fast_segments(V):
    """(S, seg) of the temperature fast path: the same S, segments not rounded."""
    S = max(16, -(-V // 8192))
    return S, -(-V // S)


def special_positions(V):
    S, seg = segments(V)
    pos = [0, V - 1]
    edges = [e for e in range(seg, V, seg)]
    for e in edges[:1] + edges[-1:]:  # the first boundary and the one before the ragged last segment
        pos += [e - 1, e]
    return list(dict.fromkeys(p for p in pos if 0 <= p < V))


def ladder(family, r):
    return 4.0 - 0.25 * r if family == "A" else 6.0 - 0.125 * r


def plant_row(V, max_topk, family, gen, first=()):
    """-> (row fp32 [V], planted positions by ladder rank).  `first`: positions that take ladder ranks 1, 2, ..."""
    n = min(max_topk + 4, V)
    if family == "A":
        row = -30.0 + 0.125 * torch.randint(-8, 9, (V,), generator=gen).float()
    else:
        row = -4.0 + 0.03125 * torch.randint(-8, 9, (V,), generator=gen).float()
    special = [p for p in special_positions(V) if p not in first]
    taken = set(special) | set(first)
    rest = [int(p) for p in torch.randperm(V, generator=gen).tolist() if p not in taken][: max(n - len(taken), 0)]
    # the special positions land on random ranks inside the nominal top-k, everything else on the remaining ranks
    head = min(n, 20)
    ranks = list(range(n))
    for j, p in enumerate(first):
        ranks.remove(1 + j)
    slots = [r for r in ranks if r < head]
    pick = [slots[i] for i in torch.randperm(len(slots), generator=gen).tolist()][: len(special)]
    pos = [None] * n
    for j, p in enumerate(first):
        pos[1 + j] = p
    for r, p in zip(pick, special):
        pos[r] = p
    it = iter(special[len(pick):] + rest)
    for r in range(n):
        if pos[r] is None:
            pos[r] = next(it)
    vals = [ladder(family, r) for r in range(n)]
    for r in (5, 19, max_topk - 1, max_topk + 2):  # exact ties: rank r + 1 takes rank r's value
        if r + 1 < n:
            vals[r + 1] = vals[r]
    row[torch.tensor(pos)] = torch.tensor(vals)
    assert torch.equal(row, row.bfloat16().float())
    return row, pos


class State:
    """The first R = min(V, max_topk + 2) ranks of one row: token ids, float64 g / p / exclusive cumulative c."""

    def __init__(self, row, flags, rp, T, policy, kb, max_topk):
        w = processed(row, flags, rp, T)
        order = torch.sort(w, descending=True, stable=True)[1]
        R = min(w.numel(), max_topk + 2)
        self.tok = order[:R].tolist()
        self.rank_of = {t: r for r, t in enumerate(self.tok)}
        self.nreal = min(kb, w.numel())
        w64 = w.double()
        top = w64[order[:R]]
        if policy == 2:
            g = top - torch.logsumexp(top[: self.nreal], 0)
        elif policy == 1:
            g = top - torch.logsumexp(w64, 0)
        else:
            g = top
        self.g = g.tolist()
        self.p = g.exp().tolist() if policy else None
        self.c = [0.0] * R
        if policy:
            for r in range(1, R):
                self.c[r] = self.c[r - 1] + self.p[r - 1]

    def kept(self, r, topp):
        return r < self.nreal and (r == 0 or topp <= 0 or self.c[r] < topp)

    def sharp(self, r, topp):
        """rank r's top-p decision is at least M (relative) away from its threshold"""
        return not (0 < r < self.nreal and topp > 0) or abs(topp - self.c[r]) >= M * self.c[r]


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def processed(row, flags, rp, T):
    """repetition penalty, then temperature, in fp32 exactly as oracle/sampler.py applies them"""
    w = row.float().clone()
    if flags is not None and rp > 0:
        r = f32(rp)
        pos, neg = flags & (w > 0), flags & (w <= 0)
        w[pos] = w[pos] * (1.0 / r)
        w[neg] = w[neg] * r
    if T > 0:
        w = w / f32(T)
    return w


def unpack_bits(mask_row, V):
    bits = torch.zeros(mask_row.numel() * 8, dtype=torch.bool)
    for bit in range(8):
        bits[bit::8] = ((mask_row >> bit) & 1).bool()
    return bits[:V]


def effective_topk(topk, max_topk):
    return max_topk if topk <= 0 or topk > max_topk else topk


def build_case(rows, requests, *, max_topk, cfg, gen, tensors, topk_dtype=torch.int32, name=""):
    """rows: list of fp32 logits rows; requests: list of (row index, kind, a, b).  Returns the case dict: the arguments
    of one fused_sampler call (CPU tensors), the intended tokens `expect` [B], `kind` / `what` per row, and - with a
    penalty - the intended mask after write-back."""
    V = rows[0].numel()
    policy, topk_cfg, topp_cfg, T, rp = cfg["policy"], cfg["topk"], cfg["topp"], cfg["T"], cfg["rp"]
    penalty = rp > 0
    nreq = len(requests)
    if penalty:
        max_bs = nreq + 3
        mask = torch.randint(0, 256, (max_bs, (V + 7) // 8), generator=gen).to(torch.uint8)
        slots = torch.randperm(max_bs, generator=gen).tolist()
    cache = {}
    out = []  # (row index, noise token, noise value, topp, topk, kind, what, expect, slot)
    nslot = 0
    for ri, kind, a, b in requests:
        topk_row = a if kind == "sweep" else topk_cfg
        kb = effective_topk(topk_row, max_topk)
        slot = None
        if penalty:
            slot = slots[nslot]
        for _ in range(200):
            if penalty:
                st = State(rows[ri], unpack_bits(mask[slot], V), rp, T, policy, kb, max_topk)
            else:
                key = (ri, kb)
                if key not in cache:
                    cache[key] = State(rows[ri], None, rp, T, policy, kb, max_topk)
                st = cache[key]
            spec = _probe(st, kind, a, b, topp_cfg)
            if spec is None or spec != "redraw":
                break
            assert penalty, (name, kind, a, b, "a decision falls within M of its threshold: change the planted row")
            mask[slot] = torch.randint(0, 256, ((V + 7) // 8,), generator=gen).to(torch.uint8)
        else:
            raise AssertionError((name, kind, a, b, "no mask row clears the margin"))
        if spec is None:
            continue
        nslot += 1
        tok, val, topp_row, expect, what = spec
        out.append((ri, tok, val, topp_row, topk_row, kind, what, expect, slot))
    B = len(out)
    assert B > 0, name
    logits = torch.stack([rows[o[0]] for o in out])
    noise = torch.zeros(B, V)
    for b, o in enumerate(out):
        noise[b, o[1]] = o[2]
    expect = torch.tensor([o[7] for o in out], dtype=torch.int32).view(B, 1)
    case = dict(name=name, V=V, B=B, max_topk=max_topk, logits=logits, gumbel_noise=noise, expect=expect,
                kind=[o[5] for o in out], what=[o[6] for o in out], softmax_policy=policy, penalty_mask=None, slot_id=None,
                expect_mask=None, cfg=cfg)
    per_row_topp = any(o[5] == "topp" for o in out)
    per_row_topk = any(o[5] == "sweep" for o in out)
    case["topp"] = torch.tensor([o[3] for o in out], dtype=torch.float32) if per_row_topp or (tensors and topp_cfg > 0) else topp_cfg
    case["topk"] = torch.tensor([o[4] for o in out], dtype=topk_dtype) if per_row_topk or tensors else topk_cfg
    case["temperature"] = torch.full((B,), T) if tensors and T > 0 else T
    case["repetition_penalty"] = torch.full((B,), rp) if tensors and rp > 0 else rp
    if penalty:
        case["penalty_mask"] = mask
        case["slot_id"] = torch.tensor([o[8] for o in out], dtype=torch.int32)
        em = mask.clone()
        for o in out:
            em[o[8], o[7] // 8] |= 1 << (o[7] % 8)
        case["expect_mask"] = em
    return case


def _probe(st, kind, a, b, topp_cfg):
    """-> (noise token, noise value, topp of the row, intended token, description), None (no such probe in this row's
    state) or "redraw" (a decision is not sharp)."""
    R = len(st.tok)
    if kind in ("member", "sweep", "token"):
        if kind == "member":
            r = a
        elif kind == "sweep":
            r = a - 1 if b == "in" else a
        else:
            r = st.rank_of.get(a)
            if r is None or not st.kept(r, topp_cfg):
                return "redraw"
        if r >= R or not math.isfinite(st.g[r]):
            return None
        if not st.sharp(r, topp_cfg):
            return "redraw"
        kept = st.kept(r, topp_cfg)
        return st.tok[r], BIG, topp_cfg, st.tok[r] if kept else st.tok[0], (kind, a, b, "rank", r, "kept" if kept else "cut")
    if kind == "score":
        i, side = a, b
        if i >= st.nreal:
            return None
        if not st.sharp(i, topp_cfg):
            return "redraw"
        if not st.kept(i, topp_cfg) or not math.isfinite(st.g[i]):
            return None
        d = st.g[0] - st.g[i]
        return st.tok[i], d + (M if side > 0 else -M), topp_cfg, st.tok[i] if side > 0 else st.tok[0], ("score", i, side)
    if kind == "topp":
        r, side = a, b
        if r >= st.nreal or not st.c[r] > 0 or not math.isfinite(st.g[r]):
            return None
        tp = st.c[r] * (1 + M if side > 0 else 1 - M)
        return st.tok[r], BIG, tp, st.tok[r] if side > 0 else st.tok[0], ("topp", r, side)
    raise ValueError(kind)


def probe_requests(V, max_topk, cfg, kinds, row=0):
    kb = effective_topk(cfg["topk"], max_topk)
    req = []
    if "member" in kinds:
        req += [(row, "member", r, None) for r in range(min(max_topk + 2, V))]
    if "score" in kinds:
        req += [(row, "score", i, s) for i in range(1, min(kb, V)) for s in (1, -1)]
    if "topp" in kinds and cfg["policy"] != 0:
        req += [(row, "topp", r, s) for r in range(1, min(kb, V)) for s in (1, -1)]
    return req


def sweep_requests(V, max_topk, row=0):
    req = []
    for k in range(1, max_topk + 1):
        req.append((row, "sweep", k, "in"))
        if k < max_topk:
            req.append((row, "sweep", k, "out"))
    return req


def _seed(V, max_topk, family, n):
    return torch.Generator().manual_seed(1_000_003 * V + 1009 * max_topk + 17 * n + (family == "B"))


@functools.lru_cache(maxsize=None)
def probe_case(V, max_topk, family, ci):
    """membership, score and top-p probes of configuration CONFIGS[ci]; odd configurations pass [B] tensors"""
    gen = _seed(V, max_topk, family, ci)
    row, _ = plant_row(V, max_topk, family, gen)
    cfg = CONFIGS[ci]
    return build_case([row], probe_requests(V, max_topk, cfg, ("member", "score", "topp")), max_topk=max_topk, cfg=cfg,
                      gen=gen, tensors=bool(ci & 1), name="probe V=%d K=%d %s cfg%d" % (V, max_topk, family, ci))


SWEEP_CONFIGS = (dict(policy=0, topk=0, topp=0.0, T=0.0, rp=0.0), dict(policy=1, topk=0, topp=0.9, T=0.0, rp=0.0))


@functools.lru_cache(maxsize=None)
def sweep_case(V, max_topk, which, with_members=False):
    """which 0: policy 0, int32 topk, family A.  which 1: policy 1 with a scalar topp, int64 topk, family B."""
    family = "AB"[which]
    gen = _seed(V, max_topk, family, 50 + which)
    row, _ = plant_row(V, max_topk, family, gen)
    cfg = SWEEP_CONFIGS[which]
    req = sweep_requests(V, max_topk)
    if with_members:
        req = probe_requests(V, max_topk, cfg, ("member",)) + req
    return build_case([row], req, max_topk=max_topk, cfg=cfg, gen=gen, tensors=False,
                      topk_dtype=(torch.int32, torch.int64)[which],
                      name="sweep V=%d K=%d %s%s" % (V, max_topk, family, " + members" if with_members else ""))


@functools.lru_cache(maxsize=None)
def masked_segments_case(max_topk=32):
    """policy 1, family B, V = 8200: whole leading, trailing and middle segments at -inf; membership and top-p probes"""
    V = 8200
    S, seg = segments(V)
    gen = _seed(V, max_topk, "B", 60)
    cfg = CONFIGS[3]
    rows, req = [], []
    for i, (lo, hi) in enumerate(((0, 4 * seg), (7 * seg, V), (2 * seg, 8 * seg))):
        row, _ = plant_row(V, max_topk, "B", gen)
        row[lo:hi] = float("-inf")
        rows.append(row)
        req += probe_requests(V, max_topk, cfg, ("member", "topp"), row=i)
    return build_case(rows, req, max_topk=max_topk, cfg=cfg, gen=gen, tensors=True, name="masked segments")


@functools.lru_cache(maxsize=None)
def writeback_case():
    """V = 8200 (mask rows of 1025 bytes): token V - 1 wins in slot max_bs - 1, tokens 8k and 8k + 7 win in other rows,
    the rest of the batch are the membership and score probes of the penalty configuration"""
    V, max_topk = 8200, 32
    gen = _seed(V, max_topk, "A", 70)
    k = int(torch.randint(1, V // 8 - 1, (1,), generator=gen))
    first = (8 * k, 8 * k + 7)
    row, _ = plant_row(V, max_topk, "A", gen, first=first)
    cfg = dict(policy=0, topk=20, topp=0.0, T=0.0, rp=1.25)
    req = [(0, "token", V - 1, None), (0, "token", first[0], None), (0, "token", first[1], None)]
    req += probe_requests(V, max_topk, cfg, ("member", "score"))
    case = build_case([row], req, max_topk=max_topk, cfg=cfg, gen=gen, tensors=False, name="write-back")
    # move the first row (token V - 1) into the last slot: swap the two slots' mask rows and ids
    mask, slot = case["penalty_mask"], case["slot_id"]
    last, s0 = mask.shape[0] - 1, int(slot[0])
    if s0 != last:
        for m in (mask, case["expect_mask"]):
            tmp = m[last].clone()
            m[last] = m[s0]
            m[s0] = tmp
        other = (slot == last).nonzero().flatten().tolist()
        slot[0] = last
        for b in other:
            slot[b] = s0
    assert int(case["expect"][0]) == V - 1 and case["expect"][1:3].flatten().tolist() == list(first)
    return case


def small_cases(only=None):
    for V in SMALL_V if only is None else (only,):
        for K in MAX_TOPK:
            for family in "AB":
                for ci in range(len(CONFIGS)):
                    yield probe_case(V, K, family, ci)
            for which in (0, 1):
                yield sweep_case(V, K, which)


def product_cases():
    yield sweep_case(120832, 32, 1, True)
    yield sweep_case(151936, 64, 0, True)


def all_cases(only=None):
    """every case test_sampler_needles.py sends to the GPU with planted noise (only: one of SMALL_V, or 0 for the rest)"""
    if only != 0:
        yield from small_cases(only)
    if only:
        return
    yield masked_segments_case()
    yield writeback_case()
    yield from product_cases()


def sampler_kwargs(case):
    return {k: case[k] for k in ("penalty_mask", "slot_id", "repetition_penalty", "temperature", "softmax_policy", "topk",
                                 "topp", "max_topk", "gumbel_noise")}


def oracle_answer(case, fn=orc.ref_fused_sampler, **extra):
    """fn (the oracle, or a variant of it) on the case -> (tokens [B, 1], expected mask or None).  The oracle's top-k
    wants V >= topk; a narrower row is widened with -inf logits, zero noise and clear mask bits, which states the same
    distribution (the kernel treats the candidates it lacks the same way: score -inf, probability 0)."""
    kw = sampler_kwargs(case)
    logits = case["logits"]
    V = case["V"]
    if kw["penalty_mask"] is not None:
        kw["penalty_mask"] = kw["penalty_mask"].clone()
    if V < case["max_topk"] + 1:
        W = 72
        logits = torch.cat([logits, torch.full((case["B"], W - V), float("-inf"))], 1)
        kw["gumbel_noise"] = torch.cat([kw["gumbel_noise"], torch.zeros(case["B"], W - V)], 1)
        if kw["penalty_mask"] is not None:
            pm = kw["penalty_mask"]
            kw["penalty_mask"] = torch.cat([pm, torch.zeros(pm.shape[0], W // 8 - pm.shape[1], dtype=torch.uint8)], 1)
    tok, mask = fn(logits, **kw, **extra)
    if mask is not None:
        mask = mask[:, : (V + 7) // 8].contiguous()
    return tok, mask


# ---- temperature fast path: the arg-max at every segment edge ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fast_path_case(V):
    """One row per position: first and last element of every fast-path segment, and V - 1.  The row's winner sits there,
    the runner-up across the segment boundary; draft = winner makes the runner-up win."""
    S, seg = fast_segments(V)
    pos = []
    for s in range(S):
        lo, hi = s * seg, min(V, (s + 1) * seg)
        if lo < hi:
            pos += [lo, hi - 1]
    pos = list(dict.fromkeys(pos + [V - 1]))
    B = len(pos)
    gen = _seed(V, 0, "A", 80)
    logits = torch.randn(B, V, generator=gen).bfloat16().float()
    noise = orc.gumbel0_like(logits, gen)
    runner = []
    for b, p in enumerate(pos):
        q = p - 1 if (p % seg == 0 and p > 0) else (p + 1 if p + 1 < V else 0)
        if p == 0:
            q = V - 1
        logits[b, p], logits[b, q] = 96.0, 64.0
        runner.append(q)
    temperature = torch.rand(B, generator=gen) * 1.5 + 0.3
    return dict(V=V, B=B, logits=logits, gumbel_noise=noise, temperature=temperature,
                winner=torch.tensor(pos, dtype=torch.int32).view(B, 1), runner=torch.tensor(runner, dtype=torch.int32).view(B, 1))


# ---- self-drawn noise on the top-k path ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def own_noise_case():
    """V = 4096, B = 4, policy 2, topk 8 and a topp that leaves 5 or 6 tokens.  -> logits, kwargs, and per row the kept
    tokens with their renormalised float64 probabilities."""
    V, B, max_topk, topk, topp = 4096, 4, 32, 8, 0.85
    gen = _seed(V, max_topk, "A", 90)
    rows, kept = [], []
    for b in range(B):
        row, _ = plant_row(V, max_topk, "A", gen)
        st = State(row, None, 0.0, 0.0, 2, topk, max_topk)
        ranks = [r for r in range(topk) if st.kept(r, topp)]
        assert all(st.sharp(r, topp) for r in range(topk)) and len(ranks) in (5, 6), ranks
        z = sum(st.p[r] for r in ranks)
        kept.append({st.tok[r]: st.p[r] / z for r in ranks})
        rows.append(row)
    return dict(V=V, B=B, logits=torch.stack(rows), kept=kept,
                kwargs=dict(softmax_policy=2, topk=topk, topp=topp, max_topk=max_topk))
