"""Draft-token verification of a speculative decode step (hpc.speculative_verify) against its PyTorch statement
(tests/spec_verify_ref.py): acceptance counts and tokens by equality on inputs whose every decision is wider than the bar
on p (asserted on the inputs, in float64), p itself from both sides of that bar, draft placement, ragged draft counts,
greedy requests, agreement with hpc.fused_sampler, outputs passed in and hipGraph replay, self-drawn noise, refusals of the
torch op and of the C entry, the fake."""
import ctypes
import functools
from pathlib import Path

import pytest
import torch

import spec_verify_ref as sref

ROOT = Path(__file__).resolve().parent.parent
F32, BF16 = torch.float32, torch.bfloat16


# ---- CPU: the definition, at V = 8 where every result can be written down ---------------------------------------------
def test_reference_on_a_hand_written_case():
    """Four requests, K = 2, every row log([.5 .25 .125 .0625 .03125 .015625 .0078125 .0078125]) at T = 1, so p is the
    table entry.  Noise is zero except where stated."""
    probs = torch.tensor([.5, .25, .125, .0625, .03125, .015625, .0078125, .0078125])
    logits = probs.log().repeat(12, 1)
    gum = torch.zeros(12, 8)
    draft = torch.tensor([[0, 1], [0, 1], [2, 9], [1, 0]])
    u = torch.tensor([[.4, .3], [.49, .2], [.1, .0], [.0, .9]])
    T = torch.tensor([1., 1., 1., 0.])
    # request 0: p = .5 > .4 accepts token 0; p = .25 < .3 rejects token 1 at row 1, where the noise would elect token 1
    # (masked) and then token 2: log .125 + 2 = -0.08 beats log .5 = -0.69
    gum[1, 1], gum[1, 2] = 10.0, 2.0
    # request 1: both accepted (.49 < .5, .2 < .25); the bonus row 5 has no mask, and noise elects token 5
    gum[5, 5] = 9.0
    # request 2: n_b = 1 (9 >= V ends the drafts): .1 < .125 accepts token 2, the bonus comes from row 7: plain arg-max 0
    # request 3 is greedy: token 1 is not the arg-max, so position 0 is rejected and holds the arg-max 0; noise is not used
    gum[9, 3] = 50.0
    out, acc, p = sref.ref_speculative_verify(logits, draft, T, u, gum)
    assert out.tolist() == [[0, 2, -1], [0, 1, 5], [2, 0, -1], [0, -1, -1]]
    assert acc.tolist() == [1, 2, 1, 0] and out.dtype == torch.int32 and acc.dtype == torch.int32
    assert torch.allclose(p[:2], torch.tensor([[.5, .25], [.5, .25]], dtype=torch.float64), atol=1e-7)
    assert abs(float(p[2, 0]) - .125) < 1e-7 and torch.isnan(p[2, 1]) and torch.isnan(p[3]).all()
    assert sref.num_valid(torch.tensor([[-1, 3], [3, 8], [3, 7], [8, 8]]), 8).tolist() == [0, 1, 2, 0]
    # a greedy request accepts its arg-max (token 0) and rejects anything else; then, with tokens 0-5 lowered in row 1,
    # tokens 6 and 7 tie for the maximum and the tie goes to the smaller id: 7 is rejected, 6 is accepted
    lg = probs.log().repeat(3, 1)
    o2, a2, _ = sref.ref_speculative_verify(lg, torch.tensor([[0, 7]]), 0.0, torch.zeros(1, 2), torch.zeros(3, 8))
    assert o2.tolist() == [[0, 0, -1]] and a2.tolist() == [1]
    lg[1, :6] = -9.0
    o3, a3, _ = sref.ref_speculative_verify(lg, torch.tensor([[0, 7]]), 0.0, torch.zeros(1, 2), torch.zeros(3, 8))
    assert o3.tolist() == [[0, 6, -1]] and a3.tolist() == [1]
    o4, a4, _ = sref.ref_speculative_verify(lg, torch.tensor([[0, 6]]), 0.0, torch.zeros(1, 2), torch.zeros(3, 8))
    assert o4.tolist() == [[0, 6, 0]] and a4.tolist() == [2]


def test_generator_lands_p_where_it_says():
    c = sref.make_case(1000, 8, 4, 5, F32)
    p = sref.draft_probs(c["logits"], c["draft"], c["T"])
    assert float(p.min()) > 0.19 and float(p.max()) < 0.96 and float(c["T"].min()) >= 0.3 and float(c["T"].max()) <= 1.8


# ---- CPU: the C entry refuses before any device call ---------------------------------------------------------------------
def _entry():
    from ctypes import c_float, c_int, c_int64, c_uint64, c_void_p

    lib = ctypes.CDLL(str(ROOT / "hpc-ops_amd" / "hpc" / "libhpc_amd.so"))
    fn = lib.hpc_speculative_verify_async
    fn.restype = c_int
    fn.argtypes = [c_void_p] * 4 + [c_int, c_int64] + [c_void_p] * 2 + [c_float] + [c_void_p] * 2 + [c_int] * 3 + [c_uint64, c_void_p]
    ws = lib.hpc_speculative_verify_workspace_bytes
    ws.restype = c_int64
    ws.argtypes = [c_int] * 3
    return fn, ws


# The pointers are never dereferenced on the host and batch_size is 0 wherever the call is accepted: every check runs
# before the `batch_size == 0` return, so no case here can reach a launch.
_P = 4096
_OK = dict(out=_P, acc=_P, ws=_P, lg=_P, dt=0, ld=1024, dr=_P, t=None, u=None, g=None, b=0, k=3, v=1024, seed=7)
_INVALID = [dict(out=None), dict(acc=None), dict(ws=None), dict(lg=None), dict(dr=None), dict(dt=2), dict(dt=-1), dict(b=-1),
            dict(k=-1), dict(v=0), dict(ld=1016), dict(u=_P), dict(g=_P), dict(seed=0)]
_UNSUPPORTED = [dict(k=16), dict(v=1028, ld=1028), dict(v=1 << 20, ld=1 << 20), dict(b=16384), dict(b=65536, k=0)]


def _call(fn, **kw):
    a = dict(_OK, **kw)
    return fn(a["out"], a["acc"], a["ws"], a["lg"], a["dt"], a["ld"], a["dr"], a["t"], 1.0, a["u"], a["g"], a["b"], a["k"],
              a["v"], a["seed"], None)


def test_c_entry_refusals():
    fn, ws = _entry()
    assert _call(fn) == 0 and _call(fn, dt=1, t=_P) == 0 and _call(fn, u=_P, g=_P, seed=0) == 0
    assert _call(fn, k=0, dr=None) == 0 and _call(fn, k=15) == 0 and _call(fn, ld=1152) == 0
    for kw in _INVALID:
        assert _call(fn, **kw) == -2, kw
    for kw in _UNSUPPORTED:
        assert _call(fn, **kw) == -1, kw
    # 16 bytes per (row, segment) and 4 per row; 16 segments up to V = 131072, then ceil(V / 8192)
    assert ws(2, 3, 1024) == 8 * 16 * 16 + 8 * 4 and ws(1, 0, 131080) == 17 * 16 + 4 and ws(0, 3, 1024) == 0


def test_fake():
    from torch._subclasses import FakeTensorMode

    import hpc  # noqa: F401

    with FakeTensorMode():
        lg = torch.empty(20, 1024, dtype=BF16, device="cuda")
        dr = torch.empty(5, 3, dtype=torch.int64, device="cuda")
        out, acc = torch.ops.hpc_spec.speculative_verify(lg, dr, None, 0.7, None, None, 7, None, None)
        assert (tuple(out.shape), out.dtype, out.device) == ((5, 4), torch.int32, lg.device)
        assert (tuple(acc.shape), acc.dtype, acc.device) == ((5,), torch.int32, lg.device)
        o, a = torch.empty(5, 4, dtype=torch.int32, device="cuda"), torch.empty(5, dtype=torch.int32, device="cuda")
        o2, a2 = hpc.speculative_verify(lg, dr, temperature=0.7, seed=7, output_token_ids=o, num_accepted=a)
        assert o2 is o and a2 is a
        o3, a3 = hpc.speculative_verify(lg, dr, temperature=torch.empty(5, device="cuda"), seed=7)
        assert o3.shape == (5, 4) and a3.shape == (5,)


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _case(V, B, K, dtype, scalar_t, seed=0):
    """One generated case with its reference; shared between tests and never modified.  A uniform lands within the bar of
    its p about once in a thousand positions: such a seed is replaced by the next one - a property of the inputs, checked
    in float64, in which the kernel has no say."""
    for attempt in range(8):
        c = sref.make_case(V, B, K, 1234 + V + 7 * B + seed + 100000 * attempt, dtype, temperature=0.8 if scalar_t else None)
        p = sref.draft_probs(c["logits"], c["draft"], c["T"])
        if float(((c["u"].double() - p).abs() / p).min()) > 2 * sref.P_BAR:
            break
    out, acc, p = sref.ref_speculative_verify(c["logits"], c["draft"], c["T"], c["u"], c["gumbel"])
    sref.assert_decidable(p, c["u"])
    return dict(c, out=out, acc=acc, p=p)


def _padded(x, pad):
    """The same rows with a row stride of V + pad; the padding holds NaN."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=x.dtype, device=x.device)
    buf[:, : x.shape[1]] = x
    return buf[:, : x.shape[1]]


def _run(c, temperature=None, logits=None, u=None, **kw):
    import hpc

    t = c["T"].cuda() if temperature is None else temperature
    lg = c["logits"].cuda() if logits is None else logits
    out, acc = hpc.speculative_verify(lg, c["draft"].cuda(), temperature=t, uniform_samples=(c["u"] if u is None else u).cuda(),
                                      gumbel_noise=c["gumbel"].cuda(), **kw)
    return out.cpu(), acc.cpu()


# ---- GPU 1: the grid ---------------------------------------------------------------------------------------------------------
# V = 8 leaves 8 of the 16 segments empty, 1000 gives ragged segments of 63, 131080 is the first size with 17 segments
GRID = [(V, B, K) for V in (8, 1000, 1024, 8200, 131080) for B, K in ((1, 1), (3, 4), (8, 4))] + [(8200, 64, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("scalar_t", [True, False], ids=["scalarT", "tensorT"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V,B,K", GRID)
def test_grid_against_reference(V, B, K, dtype, scalar_t):
    c = _case(V, B, K, dtype, scalar_t)
    share = float(c["acc"].sum()) / max(int(c["n"].sum()), 1)
    print(f"V={V} B={B} K={K}: p {float(c['p'].min()):.3f}-{float(c['p'].max()):.3f}, accepted share {share:.2f}")
    t = 0.8 if scalar_t else None
    for pad in (0, 128):
        lg = c["logits"].cuda()
        out, acc = _run(c, temperature=t, logits=_padded(lg, pad) if pad else lg)
        assert torch.equal(acc, c["acc"]), (pad, acc.tolist(), c["acc"].tolist())
        assert torch.equal(out, c["out"]), (pad, out.tolist(), c["out"].tolist())


# ---- GPU 2: p from both sides of the bar ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [8200, 131080])
def test_p_is_sharp_from_both_sides(V, dtype):
    """Request b < 4 has u = 0 before position b and u = p64 (1 + 1e-3) at it: exactly b drafts are accepted.  Request
    4 + b has u = p64 (1 - 1e-3) at position b and 0 elsewhere: all 4 are."""
    K = 4
    c = _case(V, 8, K, dtype, False)
    p = c["p"]
    u = torch.zeros(8, K, dtype=torch.float64)
    for j in range(K):
        u[j, j] = p[j, j] * (1 + sref.P_BAR)
        u[4 + j, j] = p[4 + j, j] * (1 - sref.P_BAR)
    assert float(u.max()) < 1.0
    out, acc = _run(c, u=u.float())
    assert acc.tolist() == [0, 1, 2, 3, 4, 4, 4, 4], acc.tolist()
    rout, racc, _ = sref.ref_speculative_verify(c["logits"], c["draft"], c["T"], u.float(), c["gumbel"])
    assert torch.equal(acc, racc) and torch.equal(out, rout)


# ---- GPU 3: where the draft sits ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_draft_placement(dtype):
    V, K = 8200, 1
    seg = -(-V // 16)  # 513: segment s is [513 s, 513 (s + 1))
    places = [0, V - 1, seg - 1, seg, 15 * seg, 15 * seg - 1, 4 * seg + 100]
    B = len(places)
    draft = torch.tensor(places, dtype=torch.int64).view(B, K)
    c = sref.make_case(V, B, K, 99, dtype, draft=draft)
    rout, racc, p = sref.ref_speculative_verify(c["logits"], c["draft"], c["T"], c["u"], c["gumbel"])
    sref.assert_decidable(p, c["u"])
    out, acc = _run(c)
    assert torch.equal(acc, racc) and torch.equal(out, rout), (out.tolist(), rout.tolist())
    # all accepted, all rejected: the draft's own scaled logit decides both, and the mask must sit on the draft
    for uval, want in ((0.0, 1), (0.999, 0)):
        u = torch.full((B, K), uval)
        rout, racc, _ = sref.ref_speculative_verify(c["logits"], c["draft"], c["T"], u, c["gumbel"])
        out, acc = _run(c, u=u)
        assert acc.tolist() == [want] * B and torch.equal(out, rout)
        if not want:
            assert (out[:, 0] != draft[:, 0]).all()
    # the draft is the row's unmasked Gumbel arg-max (no lift): rejected, the recovered token is another one
    c2 = sref.make_case(V, B, K, 98, dtype, lift=False)
    rows = torch.arange(B) * (K + 1)
    top = (c2["logits"][rows].float() / c2["T"].view(-1, 1) + c2["gumbel"][rows]).argmax(-1)
    c2["draft"] = top.view(B, 1)
    u = torch.full((B, K), 0.999)
    rout, racc, p2 = sref.ref_speculative_verify(c2["logits"], c2["draft"], c2["T"], u, c2["gumbel"])
    assert float(p2.max()) < 0.9 and racc.tolist() == [0] * B
    out, acc = _run(c2, u=u)
    assert torch.equal(acc, racc) and torch.equal(out, rout) and (out[:, 0] != top).all()


# ---- GPU 4: requests with different draft counts ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [1000, 8200])
def test_ragged_drafts(V, dtype):
    K = 4
    draft = torch.tensor([[-1, 5, 6, 7], [V, 5, 6, 7], [11, -1, 6, 7], [12, V + 5, 6, 7], [13, 14, 15, 16], [17, 18, 19, V - 1],
                          [3, 4, -7, 2], [-1, -1, -1, -1]], dtype=torch.int64)
    B = draft.shape[0]
    c = sref.make_case(V, B, K, 41, dtype, draft=draft)
    assert c["n"].tolist() == [0, 0, 1, 1, 4, 4, 2, 0]
    poisoned = c["logits"].clone()
    for b in range(B):
        poisoned[b * (K + 1) + int(c["n"][b]) + 1 : (b + 1) * (K + 1)] = float("nan")
    for u in (c["u"], torch.zeros(B, K)):  # drawn uniforms, and every draft accepted: the bonus row is row n_b
        rout, racc, p = sref.ref_speculative_verify(c["logits"], draft, c["T"], u, c["gumbel"])
        if u is c["u"]:
            sref.assert_decidable(p, u)
        else:
            assert torch.equal(racc.long(), c["n"])
        out, acc = _run(c, u=u)
        assert torch.equal(acc, racc) and torch.equal(out, rout), (out.tolist(), rout.tolist())
        out2, acc2 = _run(c, u=u, logits=poisoned.cuda())  # rows past n_b are not read
        assert torch.equal(acc2, racc) and torch.equal(out2, rout)


# ---- GPU 5: greedy requests ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("V", [1000, 8200])
def test_greedy(V):
    """bf16 rows of four distinct values: every row's maximum is shared by about V / 4 tokens, so the tie rule decides.
    Drafts are the arg-max (accepted), a later token holding the same value (rejected), or a random token."""
    B, K = 6, 4
    g = torch.Generator().manual_seed(3)
    logits = torch.randint(0, 4, (B * (K + 1), V), generator=g).to(BF16)
    first = logits.float().argmax(-1).view(B, K + 1)[:, :K]
    draft = first.clone()
    for b in range(B):
        r = b * (K + 1) + b % K
        tied = torch.nonzero(logits[r] == logits[r].max()).flatten()
        assert tied.numel() > 8 and int(tied[0]) == int(first[b, b % K])
        draft[b, b % K] = tied[1 + b] if b < 4 else torch.randint(0, V, (1,), generator=g)
    draft[5, 0] = first[5, 0]  # request 5 has its miss at position 1; request 4 (position 0) a random token
    u = torch.rand(B, K, generator=g)
    gum = sref.gumbel_like(logits.shape, g)
    c = dict(logits=logits, draft=draft, u=u, gumbel=gum)
    for T in (0.0, torch.tensor([0.0, 0.9, 0.0, 0.0, 1.3, 0.0])):
        rout, racc, p = sref.ref_speculative_verify(logits, draft, T, u, gum)
        sref.assert_decidable(p, u)
        if not isinstance(T, torch.Tensor):
            assert racc[:4].tolist() == [0, 1, 2, 3]
        out, acc = _run(c, temperature=T if not isinstance(T, torch.Tensor) else T.cuda())
        assert torch.equal(acc, racc) and torch.equal(out, rout), (out.tolist(), rout.tolist())
    # all drafts are the arg-max: all accepted, the bonus token is the arg-max of the last row
    rout, racc, _ = sref.ref_speculative_verify(logits, first, 0.0, u, gum)
    assert racc.tolist() == [K] * B
    out, acc = _run(dict(c, draft=first), temperature=0.0)
    assert torch.equal(acc, racc) and torch.equal(out, rout)


# ---- GPU 6: the existing sampler op ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_agrees_with_fused_sampler(dtype):
    import hpc

    V, B = 8200, 5
    c = sref.make_case(V, B, 0, 17, dtype)
    lg, t, gn = c["logits"].cuda(), c["T"].cuda(), c["gumbel"].cuda()
    out, acc = hpc.speculative_verify(lg, c["draft"].cuda(), temperature=t, uniform_samples=c["u"].cuda(), gumbel_noise=gn)
    assert out.shape == (B, 1) and acc.tolist() == [0] * B
    assert torch.equal(out, hpc.fused_sampler(lg, temperature=t, gumbel_noise=gn))
    # K = 1, every draft rejected: position 0 holds what the fast path samples with that draft masked
    c = sref.make_case(V, B, 1, 18, dtype)
    lg, t, gn, dr = c["logits"].cuda(), c["T"].cuda(), c["gumbel"].cuda(), c["draft"].cuda()
    out, acc = hpc.speculative_verify(lg, dr, temperature=t, uniform_samples=torch.full((B, 1), 0.999, device="cuda"),
                                      gumbel_noise=gn)
    assert acc.tolist() == [0] * B
    want = hpc.fused_sampler(lg[0::2], temperature=t, gumbel_noise=gn[0::2].contiguous(), draft_token_ids=dr[:, 0].contiguous())
    assert torch.equal(out[:, :1], want) and (out[:, 0] != dr[:, 0].int()).all() and (out[:, 1] == -1).all()


# ---- GPU 7: outputs passed in, inputs untouched, hipGraph replay --------------------------------------------------------------------
@pytest.mark.gpu
def test_outputs_passed_in_and_graph_replay():
    import hpc

    V, B, K = 8200, 8, 4
    cs = [_case(V, B, K, BF16, False, seed=s) for s in (0, 1, 2)]
    dev = [{k: c[k].cuda() for k in ("logits", "draft", "T", "u", "gumbel")} for c in cs]
    out = torch.full((B, K + 1), 12345, dtype=torch.int32, device="cuda")
    acc = torch.full((B,), 12345, dtype=torch.int32, device="cuda")
    d = dev[0]
    lg0, dr0 = d["logits"].clone(), d["draft"].clone()
    o, a = hpc.speculative_verify(d["logits"], d["draft"], temperature=d["T"], uniform_samples=d["u"], gumbel_noise=d["gumbel"],
                                  output_token_ids=out, num_accepted=acc)
    assert o is out and a is acc
    assert torch.equal(out.cpu(), cs[0]["out"]) and torch.equal(acc.cpu(), cs[0]["acc"])
    assert int((cs[0]["out"] == -1).sum()) > 0  # the -1 padding went over the poison
    assert torch.equal(d["logits"].view(torch.int16), lg0.view(torch.int16)) and torch.equal(d["draft"], dr0)

    buf = {k: v.clone() for k, v in d.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        hpc.speculative_verify(buf["logits"], buf["draft"], temperature=buf["T"], uniform_samples=buf["u"],
                               gumbel_noise=buf["gumbel"], output_token_ids=out, num_accepted=acc)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hpc.speculative_verify(buf["logits"], buf["draft"], temperature=buf["T"], uniform_samples=buf["u"],
                               gumbel_noise=buf["gumbel"], output_token_ids=out, num_accepted=acc)
    for i in (1, 2):
        for k in buf:
            buf[k].copy_(dev[i][k])
        out.fill_(12345)
        acc.fill_(12345)
        graph.replay()
        torch.cuda.synchronize()
        eo, ea = hpc.speculative_verify(dev[i]["logits"], dev[i]["draft"], temperature=dev[i]["T"], uniform_samples=dev[i]["u"],
                                        gumbel_noise=dev[i]["gumbel"])
        assert torch.equal(out, eo) and torch.equal(acc, ea)
        assert torch.equal(out.cpu(), cs[i]["out"]) and torch.equal(acc.cpu(), cs[i]["acc"])


# ---- GPU 8: self-drawn noise --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_own_noise_smoke():
    import hpc

    V, B, K = 8200, 16, 3
    c = sref.make_case(V, B, K, 7, F32)
    lg, dr, t = c["logits"].cuda(), c["draft"].cuda(), c["T"].cuda()
    o1, a1 = hpc.speculative_verify(lg, dr, temperature=t, seed=42)
    o2, a2 = hpc.speculative_verify(lg, dr, temperature=t, seed=42)
    for o, a in ((o1, a1), (o2, a2)):
        o, a = o.cpu(), a.cpu()
        assert ((a >= 0) & (a <= K)).all()
        for b in range(B):
            n = int(a[b])
            assert o[b, :n].tolist() == c["draft"][b, :n].tolist() and 0 <= int(o[b, n]) < V and (o[b, n + 1 :] == -1).all()
    assert not (torch.equal(o1, o2) and torch.equal(a1, a2))  # the launch offset moved


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["likely_draft", "unlikely_draft"])
def test_own_noise_distribution(which):
    """Rejection sampling leaves the target distribution alone: with a draft that is the most likely live token, or the
    least likely one, out[:, 0] follows softmax(logits) (total variation < 0.1 at 2000 draws, the bar of
    test_sampler.py::test_temperature_distribution at the same count) and the drafts are accepted with probability
    p_d (within 0.05: the binomial sigma at 2000 draws is at most 0.011 per request, below 0.006 over the batch)."""
    import hpc

    g = torch.Generator().manual_seed(1234)
    V, B, K, L, N = 1024, 4, 1, 16, 2000
    live = torch.stack([torch.randperm(V, generator=g)[:L] for _ in range(B)])
    logits = torch.full((B * (K + 1), V), -20.0)
    for b in range(B):
        logits[2 * b, live[b]] = torch.randn(L, generator=g) * 2.0 + 3.0
        logits[2 * b + 1, live[b]] = torch.randn(L, generator=g) * 2.0 + 3.0
    target = torch.softmax(logits[0::2].double(), -1)
    vals = logits[0::2].gather(1, live)
    pick = vals.argmax(-1) if which == "likely_draft" else vals.argmin(-1)
    draft = live.gather(1, pick.view(B, 1))
    p_d = target.gather(1, draft).flatten()
    dl, dd = logits.cuda(), draft.cuda()
    counts = torch.zeros(B, V, device="cuda")
    accepted = torch.zeros(B, device="cuda")
    one = torch.ones(B, 1, device="cuda")
    for _ in range(N):
        out, acc = hpc.speculative_verify(dl, dd, temperature=1.0, seed=42)
        counts.scatter_add_(1, out[:, :1].to(torch.int64), one)
        accepted += acc
    tv = 0.5 * (counts.cpu().double() / N - target).abs().sum(-1)
    rate = accepted.cpu().double() / N
    print(f"{which}: p_d {p_d.tolist()}, accepted {rate.tolist()}, tv {tv.tolist()}")
    assert (tv < 0.1).all(), tv.tolist()
    assert ((rate - p_d).abs() < 0.05).all(), (rate.tolist(), p_d.tolist())
    assert abs(float(rate.mean() - p_d.mean())) < 0.05


# ---- GPU 9: refusals of the torch op --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_error_paths():
    import hpc

    V, B, K = 1024, 2, 3
    dev = "cuda"
    lg = torch.randn(B * (K + 1), V, device=dev)
    dr = torch.randint(0, V, (B, K), device=dev)
    u, gn = torch.rand(B, K, device=dev), torch.zeros(B * (K + 1), V, device=dev)
    hpc.speculative_verify(lg, dr, uniform_samples=u, gumbel_noise=gn)
    with pytest.raises(RuntimeError, match="both be provided or both be omitted"):
        hpc.speculative_verify(lg, dr, uniform_samples=u, seed=42)
    with pytest.raises(RuntimeError, match="both be provided or both be omitted"):
        hpc.speculative_verify(lg, dr, gumbel_noise=gn, seed=42)
    with pytest.raises(RuntimeError, match="seed must be > 0"):
        hpc.speculative_verify(lg, dr)
    with pytest.raises(RuntimeError, match="draft_token_ids dtype must be int64"):
        hpc.speculative_verify(lg, dr.int(), seed=42)
    with pytest.raises(RuntimeError, match="logits rows must be"):
        hpc.speculative_verify(lg[:-1], dr, seed=42)
    with pytest.raises(RuntimeError, match="num_draft must be <= 15"):
        hpc.speculative_verify(torch.randn(17, V, device=dev), torch.zeros(1, 16, dtype=torch.int64, device=dev), seed=42)
    with pytest.raises(RuntimeError, match="unsupported vocab_size"):
        hpc.speculative_verify(torch.randn(B * (K + 1), V + 4, device=dev), dr, seed=42)
    out, acc = hpc.speculative_verify(lg[:0], dr[:0], seed=42)  # B == 0: empty tensors, no launch
    assert out.shape == (0, K + 1) and acc.shape == (0,) and out.dtype == torch.int32
