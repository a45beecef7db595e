"""What the planted-noise sampler probes (tests/sampler_needles.py) are worth - CPU only, no GPU needed.

1. The probes' intended answers, stated in float64, are the fp32 oracle's answers (oracle/sampler.py) on every row of
   every case test_sampler_needles.py runs, and the margin M = 1e-3 the two-sided probes are built with is at least 16 x
   the distance between the oracle's fp32 scores / cumulative probabilities and their float64 statement.
   Measured over the 12722 probe rows: max |g32 - g64| = 1.29e-6, max |c32 - c64| / c64 = 1.09e-6 (both at V = 8200);
   M is 775 x the larger.
2. Eleven plausible kernel bugs, restated as variants of the oracle (ref_variant below - they live here, not in
   oracle/), each change the answer of probe rows of the kind meant for them.  Rows changed, of the 12141 rows of
   sampler_needles.small_cases() (in brackets: rows of the kind and configuration meant for the mutant):
       top-k one too small (topk-1)                               1181  (518 member / sweep)
       policy 1: top-k probabilities renormalised before top-p     486  (152 topp, family B)
       temperature not applied                                    1146  (412 score, T configurations)
       penalty on non-positive logits divides                       34  (17 score, family A with a penalty)
       top-k one too large (topk+1)                               1097  (527 member / sweep)
       top-p cut one rank early (cumsum < p)                      1218  (1095 topp)
       top-p cut one rank late                                    1179  (1111 topp)
       penalty bit order reversed in a byte                       1525  (1161 score / member, penalty configurations)
       policy 2 softmax over max_topk instead of topk              649  (608 topp, policy 2)
       ties to the larger id                                       352  (71 member)
       topk ignored (always max_topk)                             1830  (1222 member / sweep)
3. Why the probes exist: four of these mutants return the oracle's tokens on every input of
   test_sampler.py::test_topk_topp_softmax_matrix.
"""
import pytest
import torch

import sampler_needles as sn
from oracle import sampler as orc

MUTANTS = ("topk-1", "renorm-before-topp", "no-temperature", "penalty-neg-divides", "topk+1", "topp-early", "topp-late",
           "penalty-bits-reversed", "softmax-over-max-topk", "ties-to-larger-id", "topk-ignored")
BLIND = MUTANTS[:4]


def ref_variant(logits, *, penalty_mask=None, slot_id=None, repetition_penalty=0.0, temperature=0.0, softmax_policy=0,
                topk=0, topp=0.0, max_topk=32, gumbel_noise, mutant=None, trace=None):
    """oracle.sampler.ref_fused_sampler, statement for statement, with one deliberate error when `mutant` names one.
    trace (a list) receives per row (idx, g fp32, exclusive cumulative probabilities fp32 or None)."""
    B, V = logits.shape
    work = logits.float().clone()

    def as_tensor(x, dtype):
        return x.to(dtype) if isinstance(x, torch.Tensor) else torch.full((B,), float(x), dtype=dtype)

    rp, temp, tp = (as_tensor(v, torch.float32) for v in (repetition_penalty, temperature, topp))
    tk = topk.to(torch.int64) if isinstance(topk, torch.Tensor) else torch.full((B,), int(topk), dtype=torch.int64)
    if penalty_mask is not None and slot_id is not None:
        for b in range(B):
            r = rp[b].item()
            if r <= 0:
                continue
            row = penalty_mask[int(slot_id[b])]
            bits = torch.zeros(row.numel() * 8, dtype=torch.bool)
            for bit in range(8):
                src = 7 - bit if mutant == "penalty-bits-reversed" else bit
                bits[bit::8] = ((row >> src) & 1).bool()
            keep = bits[:V]
            wb = work[b]
            pos, neg = keep & (wb > 0), keep & (wb <= 0)
            wb[pos] = wb[pos] * (1.0 / r)
            wb[neg] = wb[neg] * ((1.0 / r) if mutant == "penalty-neg-divides" else r)
    for b in range(B):
        t = temp[b].item()
        if t > 0 and mutant != "no-temperature":
            work[b] = work[b] / t
    if softmax_policy == 1:
        work = torch.softmax(work, dim=-1)
    if mutant == "ties-to-larger-id":  # the stable order of the reversed row ranks equal values by LARGER id
        svals, sidx = torch.sort(work.flip(-1), dim=-1, descending=True, stable=True)
        sidx = V - 1 - sidx
    else:
        svals, sidx = torch.sort(work, dim=-1, descending=True, stable=True)  # stable_topk of every row at once
    tokens = torch.empty((B, 1), dtype=torch.int32)
    for b in range(B):
        k_b = int(tk[b])
        if k_b <= 0 or k_b > max_topk or mutant == "topk-ignored":
            k_b = max_topk
        if mutant == "topk-1":
            k_b = max(k_b - 1, 1)
        if mutant == "topk+1":
            k_b = k_b + 1
        vals, idx = svals[b, :k_b], sidx[b, :k_b]
        if softmax_policy == 2:
            if mutant == "softmax-over-max-topk":
                probs = torch.softmax(svals[b, :max_topk], dim=-1)[:k_b]
            else:
                probs = torch.softmax(vals, dim=-1)
            g = probs.log()
        elif softmax_policy == 1:
            probs = vals
            g = torch.where(probs > 0, probs.log(), torch.full_like(probs, float("-inf")))
            if mutant == "renorm-before-topp":
                probs = probs / probs.sum()
        else:
            probs, g = None, vals
        keep = torch.ones(k_b, dtype=torch.bool)
        excl = None
        if tp[b].item() > 0:
            cumsum = torch.cumsum(probs, dim=-1)
            excl = cumsum - probs
            if mutant == "topp-early":
                keep = (torch.arange(k_b) == 0) | (cumsum < tp[b].item())
            elif mutant == "topp-late":
                late = torch.cat([torch.zeros(1), excl[:-1]])
                keep = (torch.arange(k_b) == 0) | (late < tp[b].item())
            else:
                keep = (torch.arange(k_b) == 0) | (excl < tp[b].item())
        if trace is not None:
            trace.append((idx, g, excl))
        key = g + gumbel_noise[b, idx]
        key = torch.where(keep, key, torch.full_like(key, float("-inf")))
        cand = (key == key.max()).nonzero(as_tuple=True)[0]
        if mutant == "ties-to-larger-id":
            best = cand[torch.argmax(idx[cand])] if cand.numel() else torch.tensor(0)
        else:
            best = cand[torch.argmin(idx[cand])] if cand.numel() else torch.tensor(0)
        tokens[b, 0] = int(idx[best])
    expected = None
    if penalty_mask is not None and slot_id is not None:
        expected = penalty_mask.clone()
        for b in range(B):
            tok = int(tokens[b, 0])
            expected[int(slot_id[b]), tok // 8] |= 1 << (tok % 8)
    return tokens, expected


def _where(case, bad):
    return [(case["name"], b, case["what"][b]) for b in bad[:8]]


def test_segments_restated():
    """the generator's segment geometry against the figures of the GPU test's table"""
    assert sn.segments(24) == (16, 256) and sn.segments(264) == (16, 256) and sn.segments(1024) == (16, 256)
    assert sn.segments(8200) == (16, 768) and sn.segments(120832) == (16, 7680) and sn.segments(151936) == (19, 8192)
    assert sn.fast_segments(8200) == (16, 513) and sn.fast_segments(120832) == (16, 7552)
    assert sn.special_positions(8200) == [0, 8199, 767, 768, 7679, 7680]
    row, pos = sn.plant_row(1024, 32, "A", torch.Generator().manual_seed(0))
    assert len(pos) == 36 and len(set(pos)) == 36 and set(sn.special_positions(1024)) <= set(pos[:20])
    order = torch.sort(row, descending=True, stable=True)[1][:36].tolist()
    assert sorted(order) == sorted(pos)
    for r in (5, 19, 31, 34):  # the tie pairs: equal values, the smaller id first
        assert row[order[r]] == row[order[r + 1]] and order[r] < order[r + 1]
    assert row[order[4]] > row[order[5]] and row[order[6]] > row[order[7]]


@pytest.mark.parametrize("V", sn.SMALL_V + (0,))
def test_probes_are_the_oracles_answers(V, capsys):
    """every probe row of every case (by vocabulary; 0: the masked-segment, write-back and product-shape cases): intended
    answer == oracle (tokens and mask), the variant without a mutant is the oracle, and M >= 16 x the largest distance
    between the oracle's fp32 g / c_r and the float64 statement"""
    rows, worst_g, worst_c = 0, 0.0, 0.0
    kinds = set()
    for case in sn.all_cases(V):
        tok, mask = sn.oracle_answer(case)
        bad = (tok != case["expect"]).flatten().nonzero().flatten().tolist()
        assert not bad, _where(case, bad)
        if case["expect_mask"] is not None:
            assert torch.equal(mask, case["expect_mask"]), case["name"]
        rows += case["B"]
        kinds |= set(case["kind"])
        if case["V"] > 10000:
            continue  # the product shapes carry membership and sweep rows only: no two-sided probe
        trace = []
        tok2, _ = sn.oracle_answer(case, ref_variant, trace=trace)
        assert torch.equal(tok2, tok), case["name"]
        cfg = case["cfg"]
        states = {}
        rows_differ = case["name"] == "masked segments"
        for b, (idx, g, excl) in enumerate(trace):
            kb = idx.numel()
            if case["penalty_mask"] is not None:
                flags = sn.unpack_bits(case["penalty_mask"][int(case["slot_id"][b])], case["V"])
                st = sn.State(case["logits"][b], flags, cfg["rp"], cfg["T"], cfg["policy"], kb, case["max_topk"])
            else:
                key = (b if rows_differ else 0, kb)
                if key not in states:
                    states[key] = sn.State(case["logits"][b], None, cfg["rp"], cfg["T"], cfg["policy"], kb, case["max_topk"])
                st = states[key]
            n = min(kb, len(st.tok), case["V"])
            assert idx[:n].tolist() == st.tok[:n], (case["name"], b)
            g64 = torch.tensor(st.g[:n], dtype=torch.float64)
            fin = torch.isfinite(g64)
            assert torch.equal(fin, torch.isfinite(g[:n]))
            if fin.any():
                worst_g = max(worst_g, float((g[:n].double() - g64)[fin].abs().max()))
            if excl is not None and n > 1:
                c64 = torch.tensor(st.c[1:n], dtype=torch.float64)
                worst_c = max(worst_c, float(((excl[1:n].double() - c64).abs() / c64).max()))
    assert kinds == ({"member", "score", "topp", "sweep"} if V else {"member", "score", "topp", "sweep", "token"})
    with capsys.disabled():
        print("\nV %d: probe rows %d   max |g32 - g64| = %.3g   max |c32 - c64| / c64 = %.3g   M = %g" % (V, rows, worst_g, worst_c, sn.M))
    assert sn.M >= 16 * max(worst_g, worst_c), (worst_g, worst_c)


# the kind of probe row that has to catch each mutant, and a narrower condition on the case where one applies
MEANT = {
    "topk-1": (("member", "sweep"), None),
    "renorm-before-topp": (("topp",), lambda c: c["cfg"]["policy"] == 1 and " B " in c["name"]),
    "no-temperature": (("score",), lambda c: c["cfg"]["T"] > 0),
    "penalty-neg-divides": (("score",), lambda c: c["cfg"]["rp"] > 0 and " A " in c["name"]),
    "topk+1": (("member", "sweep"), None),
    "topp-early": (("topp",), None),
    "topp-late": (("topp",), None),
    "penalty-bits-reversed": (("score", "member"), lambda c: c["cfg"]["rp"] > 0),
    "softmax-over-max-topk": (("topp",), lambda c: c["cfg"]["policy"] == 2),
    "ties-to-larger-id": (("member",), None),
    "topk-ignored": (("member", "sweep"), None),
}


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_is_caught(mutant, capsys):
    cases = list(sn.small_cases())
    total = sum(c["B"] for c in cases)
    kinds, cond = MEANT[mutant]
    changed = meant = 0
    for case in cases:
        if mutant == "no-temperature" and not case["cfg"]["T"] > 0:
            continue  # the mutant is the oracle itself on such a case
        if mutant in ("penalty-neg-divides", "penalty-bits-reversed") and not case["cfg"]["rp"] > 0:
            continue
        tok, _ = sn.oracle_answer(case, ref_variant, mutant=mutant)
        diff = (tok != case["expect"]).flatten()
        changed += int(diff.sum())
        if cond is None or cond(case):
            meant += sum(1 for b in diff.nonzero().flatten().tolist() if case["kind"][b] in kinds)
    with capsys.disabled():
        print("\n   %-24s %5d of %d   (%d on %s rows)" % (mutant, changed, total, meant, " / ".join(kinds)))
    assert meant > 0, (mutant, changed)


def test_blind_mutants_on_the_random_matrix():
    """the inputs of test_sampler.py::test_topk_topp_softmax_matrix (random logits, random noise, one token per row) do
    not tell these four mutants from the oracle"""
    from test_sampler import V0, _gen

    seen = 0
    for batch_size in (1, 4):
        for max_topk, topk_val in ((32, 20), (64, 50)):
            for policy, topp_val in ((0, 0.0), (1, 0.9), (2, 0.9), (2, 0.3)):
                g = _gen(1234 + max_topk + topk_val + int(topp_val * 10))
                logits = torch.randn(batch_size, V0, generator=g)
                gumbel = orc.gumbel0_like(logits, g)
                kw = dict(softmax_policy=policy, topk=torch.full((batch_size,), topk_val, dtype=torch.int32),
                          topp=torch.full((batch_size,), topp_val) if topp_val > 0 else 0.0, max_topk=max_topk,
                          gumbel_noise=gumbel)
                ref, _ = orc.ref_fused_sampler(logits, **kw)
                assert torch.equal(ref_variant(logits, **kw)[0], ref)
                for mutant in BLIND[:2]:  # the other two are the oracle itself here: no temperature, no penalty
                    assert torch.equal(ref_variant(logits, mutant=mutant, **kw)[0], ref), (mutant, policy, max_topk)
                seen += batch_size
    assert seen == 40


def test_own_noise_case_kept_set():
    """the kept set the self-drawn-noise GPU test holds the kernel to is the oracle's: +1000 at a token wins iff kept"""
    case = sn.own_noise_case()
    for b in range(case["B"]):
        row = case["logits"][b : b + 1]
        top = torch.sort(row[0], descending=True, stable=True)[1][:10].tolist()
        got = set()
        for t in top:
            noise = torch.zeros_like(row)
            noise[0, t] = sn.BIG
            if int(orc.ref_fused_sampler(row, gumbel_noise=noise, **case["kwargs"])[0]) == t:
                got.add(t)
        assert got == set(case["kept"][b]) and len(got) in (5, 6)
        assert abs(sum(case["kept"][b].values()) - 1) < 1e-12


def test_fast_path_case():
    for V in (8200,):
        case = sn.fast_path_case(V)
        S, seg = sn.fast_segments(V)
        assert case["B"] == 2 * S and {0, seg - 1, seg, V - 1} <= set(case["winner"].flatten().tolist())
        ref = orc.ref_temperature_sample(case["logits"], case["temperature"], case["gumbel_noise"])
        assert torch.equal(ref, case["winner"])
        ref = orc.ref_temperature_sample(case["logits"], case["temperature"], case["gumbel_noise"], case["winner"].flatten().long())
        assert torch.equal(ref, case["runner"])
