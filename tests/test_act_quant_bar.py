"""hpc.act_mul_and_quant (both `use_bf16_mul`), hpc.masked_act_mul_and_quant and hpc.masked_act_mul_and_blockwise_quant
against the float64 statements of tests/quant_ref.py at half an e4m3 ulp plus ACT_SLACK (tests/utils.py::quant_close):
`inter` on both sides of the 128-column block and of the kernel's 8-column chunk, planted gates where the exponential
overflows or underflows, scales of either sign and one that saturates, masked rows byte for byte.

CPU: a model of the device formula passes and its worst excess - the figure ACT_SLACK is a margin on - is printed; five
planted errors each fail (the neighbouring block's scale in two forms: returned, and used for the codes only).
Measured on the MI355X, worst excess: below zero for act_mul_and_quant and the masked form on the fp32 path (no element
beyond half an ulp), 4.0e-8 = 0.021 x ACT_SLACK on the bf16 path with at most 0.05 % of the elements on the second candidate
of the tie rule (0.78 % ambiguous); blockwise scale 1.64e-7 = 0.086 x ACT_SLACK, blockwise codes below zero."""
import math

import pytest
import torch

import quant_ref as qr
from utils import ACT_SLACK, quant_close, quant_excess, ulp_e4m3

F8 = torch.float8_e4m3fn
ROWS = qr.ACT_EXPERTS * qr.ACT_PER_EXPERT  # 192 = 48 * 4


def _either(targets, got, label):
    """quant_close against one target, or - the bf16 path's tie rule (quant_ref.silu_mul_ref64) - against either of two:
    -> (met, worst excess, share of the elements that meet the bar on the second candidate only)"""
    if len(targets) == 1:
        return quant_close(targets[0], got, ulp_e4m3, ACT_SLACK, label), float(quant_excess(targets[0], got, ulp_e4m3).max()), 0.0
    first, second = (quant_excess(t, got, ulp_e4m3) for t in targets)
    ex = torch.minimum(first, second)
    share = float(((first > ACT_SLACK) & (second <= ACT_SLACK)).double().mean())
    worst = float(ex.max())
    ok = bool((ex <= ACT_SLACK).all())
    print(f"quant_close {label}: worst excess {worst:.3g} = {worst / ACT_SLACK:.3g} x slack, second candidate taken by "
          f"{share:.4%}, ambiguous {float((targets[0] != targets[1]).double().mean()):.4%}"
          + ("" if ok else f"  FAILED: {int((ex > ACT_SLACK).sum())}/{ex.numel()} elements over"))
    if not ok:
        for i in torch.topk(ex.reshape(-1), min(10, ex.numel())).indices.tolist():
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ex.shape))
            print(f"  {idx}: got {float(got.reshape(-1)[i].float()):.9g} targets {float(targets[0].reshape(-1)[i]):.9g} / "
                  f"{float(targets[1].reshape(-1)[i]):.9g} excess {float(ex.reshape(-1)[i]):.3g}")
    return ok, worst, share


def _pertensor_targets(gate_up, scale, use_bf16_mul):
    a = qr.silu_mul_ref64(gate_up, use_bf16_mul)
    return [(v * qr.f32(scale)).clamp(-448.0, 448.0) for v in (a if use_bf16_mul else (a,))]


def _model_pertensor(gate_up, scale, use_bf16_mul, ulps=0, swap=False, cast=True):
    """the device formula in fp32 on the CPU (csrc/act_quant.h::silu_mul_scaled, then the saturating cast; cast=False: the
    fp32 value in front of the cast)"""
    gate, up = torch.chunk(gate_up.float(), 2, dim=-1)
    if swap:
        gate, up = up, gate
    s = qr.silu_device_model(gate, ulps)
    a = (s.bfloat16().float() * up).bfloat16().float() if use_bf16_mul else s * up
    v = (a * torch.tensor(scale, dtype=torch.float32)).clamp(-448.0, 448.0)
    return v.to(F8) if cast else v


def _model_blockwise(gate_up, eps=1e-8):
    """-> (codes, scale): csrc/fuse_moe.hip::act_mul_blockwise_quant_kernel's arithmetic in fp32 on the CPU"""
    gate, up = torch.chunk(gate_up.float(), 2, dim=-1)
    a = qr.silu_device_model(gate, 0) * up
    rows, inter = a.shape
    scale = a.view(rows, inter // 128, 128).abs().amax(-1) / 448.0
    inv = 1.0 / (scale + eps)
    return (a * inv.repeat_interleave(128, dim=1)).clamp(-448.0, 448.0).to(F8), scale


def _random_part(rows, inter):
    """the test's gates without the planted extremes: the measurement ACT_SLACK rests on is over |g| <= 8"""
    return ~qr.act_extreme_mask(rows, inter)


def test_inputs():
    for inter in qr.ACT_INTER:
        gu = qr.act_inputs(ROWS, inter)
        gate, up = torch.chunk(gu.float(), 2, dim=-1)
        rnd = _random_part(ROWS, inter)
        assert float(gate[rnd].abs().max()) <= 8.0 and (inter < 128 or float(gate[rnd].abs().max()) == 8.0)
        assert gate[0, inter - 8 :].tolist() == [0.0, 0.0, 90.0, -90.0, 9984.0, -9984.0, 88.5, -88.5]
        assert math.copysign(1.0, float(gate[0, inter - 7])) == -1.0  # the -0.0 survives
        assert up[0, inter - 8 :].eq(1).all() and up[2, inter - 8 :].eq(-1).all()
        if inter >= 128:
            a = qr.silu_mul_ref64(gu, False)
            assert not bool(a[qr.ACT_ZERO_ROW, :128].any()) and int(a[qr.ACT_LASTCOL_ROW, :128].abs().argmax()) == 127
    keep = qr.act_keep_mask()
    assert keep.sum() == 96 and bool(keep[qr.ACT_ZERO_ROW]) and bool(keep[qr.ACT_LASTCOL_ROW]) and not bool(keep[0]) and bool(keep[96])


def test_device_model_passes_and_its_excess():
    """the figure ACT_SLACK is a margin on: the fp32 device formula with the exponential off by +1 / 0 / -1 ulp, over the
    random gates of every input of this file.  Two figures: the excess of the e4m3 codes - positive only on the handful of
    elements that an fp32 error carries over an e4m3 tie, so it falls with the element count - and the excess of the fp32
    value in front of the cast (no half-ulp term), which is the model's fp32 error itself; the larger one counts."""
    worst, worst32 = 0.0, 0.0
    for inter in qr.ACT_INTER:
        gu = qr.act_inputs(ROWS, inter)
        rnd = _random_part(ROWS, inter)
        for scale in qr.ACT_SCALES:
            (t,) = _pertensor_targets(gu, scale, False)
            for ulps in (-1, 0, 1):
                got = _model_pertensor(gu, scale, False, ulps)
                assert quant_close(t, got, ulp_e4m3, ACT_SLACK, f"device model, exp {ulps:+d} ulp, inter {inter} scale {scale}")
                worst = max(worst, float(quant_excess(t[rnd], got[rnd], ulp_e4m3).max()))
                worst32 = max(worst32, float(quant_excess(t[rnd], _model_pertensor(gu, scale, False, ulps, cast=False)[rnd], None).max()))
    print(f"\ndevice model, worst excess over |g| <= 8: e4m3 codes {worst:.3g}, fp32 value {worst32:.3g}; "
          f"ACT_SLACK {ACT_SLACK:.3g} = {ACT_SLACK / max(worst, worst32):.3g} x the worst")
    worst = max(worst, worst32)
    # the constant is 4 x the measurement, rounded up to a power of two, 2^-16 at the most
    assert ACT_SLACK == min(2.0 ** -16, 2.0 ** math.ceil(math.log2(4 * worst)))


def test_device_model_passes_on_the_bf16_path_and_blockwise():
    gu = qr.act_inputs(ROWS, 2048)
    for scale in qr.ACT_SCALES:
        ok, _, share = _either(_pertensor_targets(gu, scale, True), _model_pertensor(gu, scale, True), f"bf16 path model, scale {scale}")
        assert ok and share <= 0.02
    a64 = qr.silu_mul_ref64(gu, False)
    q, s = _model_blockwise(gu)
    assert quant_close(qr.act_block_scale_ref64(a64), s, None, ACT_SLACK, "blockwise model, scale")
    assert quant_close(qr.act_block_targets(a64, s), q, ulp_e4m3, ACT_SLACK, "blockwise model, codes")


def _tiny_block():
    """gate_up [4, 256] whose products are of order 1e-6: the 1e-8 in `scale + 1e-8` is a fifth of the divisor"""
    g = torch.Generator().manual_seed(5)
    gu = torch.cat([torch.randn(4, 128, generator=g) * 2e-3, torch.randn(4, 128, generator=g) * 4e-4], dim=1).bfloat16()
    amax = qr.silu_mul_ref64(gu, False).abs().amax(-1)
    assert 2e-7 < float(amax.min()) and float(amax.max()) < 5e-6, amax
    return gu


MUTANTS = ["gate and up swapped", "one e4m3 code off on 0.1 % of the elements", "bf16 rounding omitted on the bf16 path",
           "the neighbouring block's scale, returned", "the neighbouring block's scale, used", "scale + 1e-8 omitted"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_bar_rejects_mutant(mutant):
    smallest = float("inf")
    for inter in ([2048] if "block" in mutant or "1e-8" in mutant else qr.ACT_INTER):
        gu = qr.act_inputs(ROWS, inter)
        scale = qr.ACT_SCALES[0]
        if mutant == "gate and up swapped":
            targets, good, bad = _pertensor_targets(gu, scale, False), _model_pertensor(gu, scale, False), _model_pertensor(gu, scale, False, swap=True)
        elif mutant.startswith("one e4m3 code"):
            targets, good = _pertensor_targets(gu, scale, False), _model_pertensor(gu, scale, False)
            codes = good.view(torch.uint8).clone().reshape(-1)
            pick = torch.randperm(codes.numel(), generator=torch.Generator().manual_seed(1))[: max(1, codes.numel() // 1000)]
            mag = codes[pick] & 0x7F
            codes[pick] = (codes[pick] & 0x80) | torch.where(mag >= 0x7E, mag - 1, mag + 1)  # the neighbouring code, never NaN
            bad = codes.view(F8).reshape(good.shape)
        elif mutant.startswith("bf16 rounding"):
            targets, good, bad = _pertensor_targets(gu, scale, True), _model_pertensor(gu, scale, True), _model_pertensor(gu, scale, False)
        else:
            if "1e-8" in mutant:
                gu = _tiny_block()
            a64 = qr.silu_mul_ref64(gu, False)
            q, s = _model_blockwise(gu)
            assert quant_close(qr.act_block_scale_ref64(a64), s, None, ACT_SLACK, "model, scale")
            assert quant_close(qr.act_block_targets(a64, s), q, ulp_e4m3, ACT_SLACK, "model, codes")
            if mutant.endswith("returned"):     # codes and scale agree with each other: the scale's own check sees it
                ex = quant_excess(qr.act_block_scale_ref64(a64), s.roll(1, 1), None)
            elif mutant.endswith("used"):       # the right scale returned, the codes made with the neighbour's
                inv = (1.0 / (s.roll(1, 1) + 1e-8)).repeat_interleave(128, dim=1)
                gate, up = torch.chunk(gu.float(), 2, dim=-1)
                bad = (qr.silu_device_model(gate, 0) * up * inv).clamp(-448.0, 448.0).to(F8)
                ex = quant_excess(qr.act_block_targets(a64, s), bad, ulp_e4m3)
            else:
                bad, s_bad = _model_blockwise(gu, eps=0.0)
                assert torch.equal(s, s_bad)
                ex = quant_excess(qr.act_block_targets(a64, s), bad, ulp_e4m3)
            smallest = min(smallest, float(ex.max()))
            continue
        ok, _, share = _either(targets, good, f"model, inter {inter}")
        assert ok and share <= 0.02
        ok, worst, share = _either(targets, bad, f"{mutant}, inter {inter}")
        assert not ok
        smallest = min(smallest, worst)
    print(f"{mutant}: smallest worst-excess {smallest:.3g} = {smallest / ACT_SLACK:.3g} x ACT_SLACK")
    assert smallest > ACT_SLACK


# ------------------------------------------------------------------------------------------------------------ GPU
def _check_pertensor(gu, scale, use_bf16_mul, got, rows, label):
    """the bar on `rows` (a mask) and the planted extremes by value -> (met, worst excess, second-candidate share)"""
    n, inter = got.shape
    targets = [t[rows] for t in _pertensor_targets(gu, scale, use_bf16_mul)]
    ok, worst, share = _either(targets, got[rows], label)
    ext = qr.act_extreme_mask(n, inter) & rows.unsqueeze(1)
    want = qr.act_extreme_expected(gu, scale)
    if not torch.equal(got.float()[ext], want[ext]):  # by value: -0 is 0
        print(f"{label}: planted extremes differ: got {got.float()[ext][:16].tolist()} want {want[ext][:16].tolist()}")
        ok = False
    return ok, worst, share, int((targets[0].abs() == 448.0).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("use_bf16_mul", [False, True])
@pytest.mark.parametrize("inter", qr.ACT_INTER)
def test_act_mul_and_quant_bar(inter, use_bf16_mul):
    import hpc

    failed, worst, shares, saturated = [], float("-inf"), [], 0
    for rows in (1, 3, ROWS):
        gu = qr.act_inputs(rows, inter)
        for scale in qr.ACT_SCALES:
            got = hpc.act_mul_and_quant(gu.cuda(), torch.tensor([scale]).cuda(), use_bf16_mul=use_bf16_mul).cpu()
            assert got.dtype == F8 and tuple(got.shape) == (rows, inter)
            label = f"act_mul_and_quant inter {inter} rows {rows} scale {scale} bf16 {use_bf16_mul}"
            ok, w, share, sat = _check_pertensor(gu, scale, use_bf16_mul, got, torch.ones(rows, dtype=torch.bool), label)
            worst, saturated = max(worst, w), saturated + (sat if scale == 300.0 else 0)
            shares.append(share)
            if not ok:
                failed.append(label)
    print(f"inter {inter} bf16 {use_bf16_mul}: worst excess {worst:.3g} = {worst / ACT_SLACK:.3g} x ACT_SLACK; second candidate "
          f"taken by at most {max(shares):.4%}; {saturated} saturated at scale 300")
    assert not failed, failed
    assert max(shares) <= 0.02, shares  # beyond that the tie rule would be hiding something
    assert saturated > 0


@pytest.mark.gpu
@pytest.mark.parametrize("inter", qr.ACT_INTER)
def test_masked_act_mul_and_quant_bar(inter):
    import hpc

    gu, keep = qr.act_inputs(ROWS, inter), qr.act_keep_mask()
    cnt = torch.tensor(qr.ACT_COUNTS, dtype=torch.int32)
    sentinel = torch.full((ROWS, inter), 3.0).to(F8)
    failed, worst = [], float("-inf")
    for scale in qr.ACT_SCALES:
        out = sentinel.clone().cuda()
        my = hpc.masked_act_mul_and_quant(gu.cuda(), torch.tensor([scale]).cuda(), cnt.cuda(), output=out)
        assert my.data_ptr() == out.data_ptr()
        got = my.cpu()
        label = f"masked_act_mul_and_quant inter {inter} scale {scale}"
        ok, w, _, _ = _check_pertensor(gu, scale, False, got, keep, label)
        worst = max(worst, w)
        if not ok:
            failed.append(label)
        assert torch.equal(got.view(torch.uint8)[~keep], sentinel.view(torch.uint8)[~keep]), label  # rows past the count: untouched
    print(f"masked, inter {inter}: worst excess {worst:.3g} = {worst / ACT_SLACK:.3g} x ACT_SLACK")
    assert not failed, failed


@pytest.mark.gpu
@pytest.mark.parametrize("inter", qr.ACT_INTER)
def test_masked_act_mul_and_blockwise_quant_bar(inter):
    import hpc

    gu, keep = qr.act_inputs(ROWS, inter), qr.act_keep_mask()
    cnt = torch.tensor(qr.ACT_COUNTS, dtype=torch.int32).cuda()
    if inter % 128:
        with pytest.raises(RuntimeError, match="divided by 128"):  # the entry's documented refusal (csrc/torch_moe.cpp)
            hpc.masked_act_mul_and_blockwise_quant(gu.cuda(), cnt)
        return
    q_sent, s_sent = torch.full((ROWS, inter), 3.0).to(F8), torch.full((ROWS, inter // 128), 777.0)
    q_out, s_out = q_sent.clone().cuda(), s_sent.clone().cuda()
    q, s = hpc.masked_act_mul_and_blockwise_quant(gu.cuda(), cnt, output=q_out, output_scale=s_out)
    assert q.data_ptr() == q_out.data_ptr() and s.data_ptr() == s_out.data_ptr() and q.dtype == F8 and s.dtype == torch.float32
    q, s = q.cpu(), s.cpu()
    a64 = qr.silu_mul_ref64(gu, False)
    # two independent checks: the scale against amax / 448, the codes against the scale the op itself returned
    ex_s = quant_excess(qr.act_block_scale_ref64(a64)[keep], s[keep], None)
    ex_q = quant_excess(qr.act_block_targets(a64, s)[keep], q[keep], ulp_e4m3)
    print(f"blockwise, inter {inter}: worst excess scale {float(ex_s.max()):.3g} = {float(ex_s.max()) / ACT_SLACK:.3g} x ACT_SLACK, "
          f"codes {float(ex_q.max()):.3g} = {float(ex_q.max()) / ACT_SLACK:.3g} x ACT_SLACK")
    assert quant_close(qr.act_block_scale_ref64(a64)[keep], s[keep], None, ACT_SLACK, f"blockwise scale, inter {inter}")
    assert quant_close(qr.act_block_targets(a64, s)[keep], q[keep], ulp_e4m3, ACT_SLACK, f"blockwise codes, inter {inter}")
    assert float(s[qr.ACT_ZERO_ROW, 0]) == 0.0 and not bool(q[qr.ACT_ZERO_ROW, :128].float().any())  # the all-zero block
    assert abs(float(q[qr.ACT_LASTCOL_ROW, 127].float())) == 448.0                                  # amax in the last column
    assert torch.equal(q.view(torch.uint8)[~keep], q_sent.view(torch.uint8)[~keep])
    assert torch.equal(s[~keep], s_sent[~keep])
