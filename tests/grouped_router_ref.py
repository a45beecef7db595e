"""Group-limited top-k router (hpc.grouped_topk_router): the parity definition and what the tests derive from it.

There is no reference counterpart (the reference has no router).  `ref_grouped_topk_router` is the definition: DeepSeek-V3 /
R1 and Kimi-K2 routing (sigmoid scores, correction bias, group score = sum of the group's two best, weights from the
unbiased scores, routed scaling factor) and DeepSeek-V2's (softmax scores, no bias, group score = the group's best), with
the tie rule of hpc.topk_router: smaller expert id first, and smaller group id first.

`decision` evaluates the same rule in float64 and returns the gaps a row's result hangs on, so that a test can say which
rows a correct fp32 kernel may decide differently (its exp is not torch's) and what it must still satisfy there."""
import torch


def ref_grouped_topk_router(logits, bias, topk, n_group, topk_group, scoring, renormalize, scale, dtype=torch.float32):
    """logits [m, n], bias [n] or None -> (ids int32 [m, topk] best first, weights `dtype` [m, topk])."""
    x = logits.to(dtype)
    s = torch.sigmoid(x) if scoring == "sigmoid" else torch.softmax(x, -1)     # scores
    c = s + bias.to(dtype) if bias is not None else s                          # choice scores
    m, n = c.shape
    gs = n // n_group
    cg = c.view(m, n_group, gs)
    gscore = (cg.sort(dim=-1, descending=True, stable=True).values[..., :2].sum(-1) if bias is not None
              else cg.max(-1).values)                                          # top-2 sum with a bias, max without
    gorder = gscore.sort(dim=-1, descending=True, stable=True).indices         # ties -> smaller group id
    keep = torch.zeros(m, n_group, dtype=torch.bool).scatter_(1, gorder[:, :topk_group], True)
    cm = torch.where(keep[:, :, None].expand(m, n_group, gs).reshape(m, n), c, torch.full_like(c, float("-inf")))
    ids = cm.sort(dim=-1, descending=True, stable=True).indices[:, :topk]      # ties -> smaller expert id, best first
    w = s.gather(1, ids)                                                       # weights from the UNBIASED scores
    if renormalize:
        w = w / (w.sum(-1, keepdim=True) + 1e-20)
    return ids.int(), w * scale


def _neighbour_gaps(v):
    """differences of neighbours along the last dimension of a descending tensor; -inf next to -inf counts as no gap"""
    d = v[..., :-1] - v[..., 1:]
    return torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)


def decision(logits, bias, topk, n_group, topk_group, scoring):
    """The float64 evaluation of the rule and the gaps that decide a row.  Returns a dict of
      c          [m, n]   float64 choice scores
      gscore     [m, G]   float64 group scores
      cand       [m, n]   c with the experts outside the float64 evaluation's kept groups at -inf
      gaps       [m]      smallest gap between neighbours among the first topk + 1 ordered candidates and among the
                          first topk_group + 1 ordered group scores (an exact tie is a gap of 0)
      strict     [m]      the same without the exact ties that every fp32 evaluation resolves by id alone, whatever its
                          exp rounds to.  These are: two candidates with the same logit and the same bias; and, at the
                          one place in the group order that decides what stays (between the topk_group-th group and the
                          next), two groups whose best (two best, with a bias) choice scores are the same values, or
                          whose two best are four values in [1, 2) with the same logits and biases that are multiples
                          of 2^-6 with the same sum.  (There c = s + b rounds s alone, to the grid of [1, 2), the same
                          way for every such b, so both sums are roundings of one real number.)  Any other tie of two
                          sums of different values there stays in as 0: it is exact in one rounding and a gap of an ulp
                          in another.  The order among the groups that stay decides nothing, so an exact 0 there is
                          left out whatever it comes from; a nonzero gap is not."""
    x = logits.double()
    s = torch.sigmoid(x) if scoring == "sigmoid" else torch.softmax(x, -1)
    c = s + bias.double() if bias is not None else s
    m, n = c.shape
    gs = n // n_group
    top2 = c.view(m, n_group, gs).sort(dim=-1, descending=True, stable=True).values[..., :2]
    gscore = top2.sum(-1) if bias is not None else top2[..., 0]
    gsorted, gorder = gscore.sort(dim=-1, descending=True, stable=True)
    keep = torch.zeros(m, n_group, dtype=torch.bool).scatter_(1, gorder[:, :topk_group], True)
    cand = torch.where(keep[:, :, None].expand(m, n_group, gs).reshape(m, n), c, torch.full_like(c, float("-inf")))
    csorted, corder = cand.sort(dim=-1, descending=True, stable=True)
    inf = torch.full((m, 1), float("inf"), dtype=torch.float64)
    cgap = _neighbour_gaps(csorted[:, :topk + 1])
    ggap = _neighbour_gaps(gsorted[:, :topk_group + 1])
    gaps = torch.cat([cgap, ggap, inf], 1).amin(1)
    # exact ties between equal inputs
    xo = x.gather(1, corder[:, :topk + 1])
    bo = (bias.double()[corder[:, :topk + 1]] if bias is not None else torch.zeros_like(xo))
    same_c = (xo[:, :-1] == xo[:, 1:]) & (bo[:, :-1] == bo[:, 1:])
    t2 = top2.gather(1, gorder[:, :topk_group + 1, None].expand(m, min(topk_group + 1, n_group), 2))
    same_g = (t2[:, :-1, 0] == t2[:, 1:, 0]) & ((t2[:, :-1, 1] == t2[:, 1:, 1]) if bias is not None else True)
    if bias is not None and bool((bias.double() * 64 == (bias.double() * 64).round()).all()):
        order = gorder[:, :topk_group + 1]
        xg = x.view(m, n_group, gs).gather(2, c.view(m, n_group, gs).sort(dim=-1, descending=True, stable=True).indices[..., :2])
        x2 = xg.sort(dim=-1).values.gather(1, order[:, :, None].expand(-1, -1, 2))
        in_binade = ((t2 >= 1) & (t2 < 2)).all(-1)
        same_g = same_g | ((ggap == 0) & (x2[:, :-1] == x2[:, 1:]).all(-1) & in_binade[:, :-1] & in_binade[:, 1:])
    big = torch.tensor(float("inf"), dtype=torch.float64)
    boundary = torch.zeros_like(same_g)
    boundary[:, topk_group - 1:] = True
    harmless = torch.where(boundary, same_g, ggap == 0)
    strict = torch.cat([torch.where(same_c, big, cgap), torch.where(harmless, big, ggap), inf], 1).amin(1)
    return dict(c=c, gscore=gscore, cand=cand, gaps=gaps, strict=strict)


def check_close_row(ids_row, d, r, topk, n_group, topk_group, slack=2e-5):
    """What a row that hangs on a gap of a few ulp must still satisfy: distinct ids in range, every chosen expert in a
    group whose float64 score is within `slack` of the topk_group-th best, and with a float64 choice score of at least
    the topk-th best candidate's minus `slack`."""
    n = d["c"].shape[1]
    gs = n // n_group
    ids = [int(i) for i in ids_row]
    assert len(set(ids)) == topk and all(0 <= i < n for i in ids), (r, ids)
    g_bar = d["gscore"][r].sort(descending=True).values[topk_group - 1] - slack
    c_bar = d["cand"][r].sort(descending=True).values[topk - 1] - slack
    for i in ids:
        assert d["gscore"][r, i // gs] >= g_bar, (r, i, float(d["gscore"][r, i // gs]), float(g_bar))
        assert d["c"][r, i] >= c_bar, (r, i, float(d["c"][r, i]), float(c_bar))
