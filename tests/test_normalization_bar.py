"""hpc.fused_rmsnorm_with_scale against the float64 statement (tests/quant_ref.py::rmsnorm_ref64) at half an e4m3 ulp plus
NORM_SLACK (tests/utils.py::quant_close), on needle rows at both ends of every rung of HPC_RMS_LADDER
(csrc/rmsnorm_row.h), with both `is_moe` instantiations, saturation and NaN.

CPU: the fp32 oracle (oracle/normalization.py) passes the bar on these inputs and its worst excess - the figure NORM_SLACK
is a margin on - is printed; six planted errors of an fp32 model of the kernel each fail it.
GPU: the kernel itself, e4m3 outputs included (tests/test_normalization.py checks `is_moe=False` at atol 0.15 only).
Measured on the MI355X: worst excess 2.09e-7 = 0.109 x NORM_SLACK on the fp32 output (hidden 16384), 4.4e-8 = 0.023 x on the
e4m3 outputs."""
import math

import pytest
import torch

import quant_ref as qr
from utils import NORM_SLACK, quant_close, quant_excess, ulp_e4m3

F8 = torch.float8_e4m3fn
EPS = qr.NORM_EPS


def _tpr(hidden):
    """threads per row of HPC_RMS_LADDER (csrc/rmsnorm_row.h)"""
    nvec = hidden // 8
    return 64 if nvec <= 64 else 128 if nvec <= 128 else 256


def _model(x, w, scale, mutant=None):
    """fp32 model of the kernel, (y fp32, q0 e4m3, q1 e4m3), with one planted error when `mutant` names it"""
    rows, hidden = x.shape
    xf, sq = x.float(), x.float().pow(2)
    if mutant == "last vector out of the sum":
        sq[:, hidden - 8 :] = 0
    if mutant == "one wave's stripe out of the sum":
        vec = torch.arange(hidden) // 8          # vector v is held by thread v % kTPR, wave (v % kTPR) / 64: wave 1 dropped
        sq[:, (vec % _tpr(hidden)) // 64 == 1] = 0
    eps = 0.0 if mutant == "eps omitted" else EPS
    rms = torch.rsqrt(sq.sum(-1, keepdim=True) / hidden + eps)
    if mutant == "rms of the next row":
        rms = rms.roll(-1, 0)
    y = xf * rms * w.float().reshape(1, -1)
    inv = 1.0 / torch.tensor(scale, dtype=torch.float32)
    if mutant == "scale[0] for the second output":
        inv[1] = inv[0]
    cast = qr.e4m3_truncate if mutant == "truncating e4m3 cast" else (lambda v: v.clamp(-448.0, 448.0).to(F8))
    return y, cast(y * inv[0]), cast(y * inv[1])


def _oracle(x, w, scale):
    """the pinned fp32 oracle, with the kernel's saturation (torch's own cast turns |v| > 448 into NaN)"""
    from oracle import normalization as onorm

    y = onorm.rmsnorm_fp32(x, w, EPS)
    inv = 1.0 / torch.tensor(scale, dtype=torch.float32)
    return y, (y * inv[0]).clamp(-448.0, 448.0).to(F8), (y * inv[1]).clamp(-448.0, 448.0).to(F8)


def _excess(x, w, scale, outs):
    """worst quant_excess of (y fp32, q0, q1) -> three floats"""
    y64 = qr.rmsnorm_ref64(x, w, EPS)
    t0, t1 = qr.norm_targets(y64, scale)
    return [float(quant_excess(y64, outs[0], None).max()), float(quant_excess(t0, outs[1], ulp_e4m3).max()),
            float(quant_excess(t1, outs[2], ulp_e4m3).max())]


def test_quant_excess_basics():
    t = torch.tensor([1.03, -300.0, 448.0, 0.0, 0.0, float("nan"), 0.0045, 5.0], dtype=torch.float64)
    got = torch.tensor([1.0, -288.0, 448.0, 0.0, -0.0, float("nan"), 2.0 ** -8, 5.0]).to(F8)
    assert got.view(torch.uint8)[5] == 0x7F
    ex = quant_excess(t, got, ulp_e4m3)
    assert float(ex.max()) <= 0.0 and quant_close(t, got, ulp_e4m3, NORM_SLACK, "nearest codes")
    other_nan = got.clone().view(torch.uint8)
    other_nan[5] = 0xFF                     # e4m3fn's second NaN encoding: not what the reference's cast writes
    assert float(quant_excess(t, other_nan.view(F8), ulp_e4m3)[5]) == float("inf")
    for i, v in ((0, 1.125), (1, -320.0), (2, 416.0), (3, 2.0 ** -9), (6, 2.0 ** -8 + 2.0 ** -9), (7, float("nan"))):
        bad = got.float()
        bad[i] = v
        assert not quant_close(t, bad.to(F8), ulp_e4m3, NORM_SLACK, f"element {i} moved"), i
    # an fp32 output: the slack alone
    y = torch.tensor([3.0, -1e-3, 0.0], dtype=torch.float64)
    assert quant_close(y, y.float(), None, NORM_SLACK, "fp32")
    assert not quant_close(y, (y * (1 + 4 * NORM_SLACK)).float(), None, NORM_SLACK, "fp32 moved")


def test_inputs_are_the_needles():
    for hidden in qr.NORM_HIDDEN:
        x, w = qr.norm_inputs(9, hidden)
        e = x.float().pow(2)
        assert float(e[1, : hidden - 8].sum()) == 0 and float(e[1].sum()) > 0
        v = qr.norm_lane_vector(hidden)
        assert float(e[2].sum()) == float(e[2, 8 * v : 8 * v + 8].sum()) > 0
        assert 1e-4 < float(x[3].float().abs().mean()) < 2e-3 and not bool(x[4].any())
        rms = e.mean(-1).sqrt()
        assert float(rms[5] / rms[6]) < 0.6 and float(rms[7] / rms[6]) > 1.7  # neighbours differ


def test_fp32_oracle_passes_and_its_excess():
    """the figure NORM_SLACK is a margin on, measured on every input of this file"""
    worst = [0.0, 0.0, 0.0]
    for hidden in qr.NORM_HIDDEN:
        for rows in qr.NORM_ROWS:
            x, w = qr.norm_inputs(rows, hidden)
            for scale in qr.NORM_SCALES:
                worst = [max(a, b) for a, b in zip(worst, _excess(x, w, scale, _oracle(x, w, scale)))]
    print(f"\nfp32 oracle, worst excess: fp32 output {worst[0]:.3g}, e4m3 {worst[1]:.3g} / {worst[2]:.3g}; "
          f"NORM_SLACK {NORM_SLACK:.3g} = {NORM_SLACK / max(worst):.3g} x the worst")
    # the constant is the next power of two at or above 8 x the measurement, 2^-18 at the most
    assert NORM_SLACK == min(2.0 ** -18, 2.0 ** math.ceil(math.log2(8 * max(worst))))


MUTANTS = ["rms of the next row", "last vector out of the sum", "one wave's stripe out of the sum",
           "scale[0] for the second output", "truncating e4m3 cast", "eps omitted"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_bar_rejects_mutant(mutant):
    """every planted error fails the bar at every hidden size it applies to, on the e4m3 output alone - what `is_moe=False`
    leaves to look at (the second e4m3 output for the scale mix-up; row 3, of magnitude 1e-3, for the missing eps)"""
    smallest, scale = float("inf"), qr.NORM_SCALES[0]
    for hidden in qr.NORM_HIDDEN:
        if mutant.startswith("one wave") and _tpr(hidden) == 64:
            continue  # one wave holds the whole row: there is no partial sum to lose
        x, w = qr.norm_inputs(9, hidden)
        y64 = qr.rmsnorm_ref64(x, w, EPS)
        t = qr.norm_targets(y64, scale)
        good, bad = _model(x, w, scale), _model(x, w, scale, mutant)
        which = 2 if mutant.startswith("scale[0]") else 1
        rows = slice(3, 4) if mutant == "eps omitted" else slice(None)
        assert quant_close(t[which - 1][rows], good[which][rows], ulp_e4m3, NORM_SLACK, f"model, hidden {hidden}")
        assert not quant_close(t[which - 1][rows], bad[which][rows], ulp_e4m3, NORM_SLACK, f"{mutant}, hidden {hidden}")
        smallest = min(smallest, float(quant_excess(t[which - 1][rows], bad[which][rows], ulp_e4m3).max()))
    print(f"{mutant}: smallest worst-excess over the hidden sizes {smallest:.3g} = {smallest / NORM_SLACK:.3g} x NORM_SLACK")
    assert smallest > NORM_SLACK


# ------------------------------------------------------------------------------------------------------------ GPU
def _run(x, w, scale, is_moe):
    import hpc

    out = hpc.fused_rmsnorm_with_scale(x.cuda(), w.cuda(), eps=EPS, scale=torch.tensor(scale, dtype=torch.float32).cuda(),
                                       is_moe=is_moe)
    torch.cuda.synchronize()
    return [t.cpu() for t in out] if is_moe else [None, out.cpu(), None]


def _check(x, w, scale, is_moe, outs, label):
    """-> (all bars met, number of saturated targets of the e4m3 outputs checked)"""
    y64 = qr.rmsnorm_ref64(x, w, EPS)
    t0, t1 = qr.norm_targets(y64, scale)
    assert outs[1].dtype == F8 and outs[1].shape == x.shape
    ok = quant_close(t0, outs[1], ulp_e4m3, NORM_SLACK, f"{label} e4m3")
    if is_moe:
        assert outs[0].dtype == torch.float32 and outs[2].dtype == F8
        ok = quant_close(y64, outs[0], None, NORM_SLACK, f"{label} fp32") and ok
        ok = quant_close(t1, outs[2], ulp_e4m3, NORM_SLACK, f"{label} e4m3, second scale") and ok
    return ok, int((t0.abs() == 448.0).sum()) + (int((t1.abs() == 448.0).sum()) if is_moe else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("is_moe", [False, True])
@pytest.mark.parametrize("hidden", qr.NORM_HIDDEN)
def test_fused_rmsnorm_with_scale_bar(hidden, is_moe):
    failed, saturated = [], 0
    for rows in qr.NORM_ROWS:
        x, w = qr.norm_inputs(rows, hidden)
        for scale in qr.NORM_SCALES:
            # is_moe=False reads scale[0] only: give it each of the four scales in turn
            for sc in ([scale] if is_moe else [[scale[0]] * 2, [scale[1]] * 2]):
                label = f"hidden {hidden} rows {rows} scale {sc if is_moe else sc[0]} is_moe {is_moe}"
                ok, sat = _check(x, w, sc, is_moe, _run(x, w, sc if is_moe else sc[:1], is_moe), label)
                saturated += sat
                if not ok:
                    failed.append(label)
    assert not failed, failed
    # |y| <= sqrt(hidden) * max w: at hidden 8 that is 3.6, below 448 * 0.011 = 4.9 - nothing can saturate there
    print(f"hidden {hidden}: {saturated} saturated targets")
    assert saturated > 0 or hidden == 8


@pytest.mark.gpu
def test_hidden_past_the_ladder_is_refused():
    import hpc

    x = torch.randn(3, 16392, dtype=torch.bfloat16, device="cuda")
    w = torch.rand(16392, dtype=torch.bfloat16, device="cuda")
    for is_moe in (False, True):
        with pytest.raises(RuntimeError):
            hpc.fused_rmsnorm_with_scale(x, w, scale=torch.tensor([2.5, 5.0]), is_moe=is_moe)


@pytest.mark.gpu
@pytest.mark.parametrize("is_moe", [False, True])
@pytest.mark.parametrize("hidden", [8, 520, 4104, 16384])
def test_nan_stays_in_its_row(hidden, is_moe):
    """one NaN input element: its whole row is NaN in every output (0x7f in e4m3), every other row is what it was"""
    x, w = qr.norm_inputs(9, hidden)
    scale = qr.NORM_SCALES[0]
    clean = _run(x, w, scale, is_moe)
    x = x.clone()
    x[6, hidden - 3] = float("nan")
    outs = _run(x, w, scale, is_moe)
    ok, _ = _check(x, w, scale, is_moe, outs, f"NaN in row 6, hidden {hidden} is_moe {is_moe}")  # the targets of row 6 are NaN
    assert ok
    others = torch.arange(9) != 6
    for a, b in zip(clean, outs):
        if a is not None:
            assert bool(b[6].float().isnan().all())
            assert torch.equal(a[others].view(torch.uint8), b[others].view(torch.uint8))
