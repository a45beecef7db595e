"""Golden fixtures made by running the REFERENCE's own in-file oracle functions on the CPU
(tests/golden/make_golden.py + ref_extract.py, build container only):
 * CPU: our oracle restatements reproduce the stored reference outputs (this is what pins them);
 * GPU: the HIP path, through the C-ABI, matches the stored reference outputs at the reference's tolerances.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

from utils import allclose

G = np.load(Path(__file__).resolve().parent / "golden" / "fp_golden.npz")
F8 = torch.float8_e4m3fn


def bf(name):
    return torch.from_numpy(G[name].copy()).view(torch.bfloat16)


def f8(name):
    return torch.from_numpy(G[name].copy()).view(F8)


def t(name):
    return torch.from_numpy(G[name].copy())


def _nblocks(lens, sq, P=64):
    return (lens + sq + P - 1) // P


# ---------------------------------------------------------------------------- CPU: pin the oracles
def test_oracle_rmsnorm_matches_reference_output():
    from oracle import normalization as onorm

    x, w = bf("norm_x"), bf("norm_w")
    assert torch.equal(onorm.rmsnorm_fp32(x, w, 1e-6), t("norm_y32"))
    assert torch.equal(onorm.rmsnorm_with_scale_fp8(x, w, torch.tensor(2.5), 1e-6), bf("norm_y8"))


def test_oracle_allreduce_matches_reference_output():
    from oracle import allreduce as oar

    xs = list(bf("ar_x"))
    rr, ro = oar.ref_allreduce_rmsnorm(xs, bf("ar_res"), bf("ar_w"), 1e-6)
    assert torch.equal(rr, bf("ar_out_res")) and torch.equal(ro, bf("ar_out"))


_SFQ = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def _sfq_x(tag):
    x = t(f"sfq_x_{tag}")
    return x if tag == "f32" else x.view(_SFQ[tag])


@pytest.mark.parametrize("tag", sorted(_SFQ))
def test_oracle_scaled_fp8_quant_matches_reference_output(tag):
    """Stored outputs = the reference's eager form (benchmark/fused_moe/backends/base.py:64-67) on in-range inputs;
    scale 0.25 is exact in both forms, at 1e-2 an e4m3 tie may fall on the other side (<= one code, < 0.2 %)."""
    from oracle import fuse_moe as omoe

    x = _sfq_x(tag)
    q1, _ = omoe.scaled_fp8_quant(x, torch.full((), 0.25))
    assert torch.equal(q1.view(torch.uint8), t(f"sfq_q_{tag}_1"))
    q0, _ = omoe.scaled_fp8_quant(x, torch.full((), 1e-2))
    d = (q0.view(torch.uint8).int() - t(f"sfq_q_{tag}_0").int()).abs()
    assert d.max() <= 1 and (d != 0).float().mean() < 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(_SFQ))
def test_hip_scaled_fp8_quant_matches_reference_output(tag):
    import hpc

    x = _sfq_x(tag).cuda()
    q1, s1 = hpc.scaled_fp8_quant(x, torch.full((), 0.25, device="cuda"))
    assert torch.equal(q1.cpu().view(torch.uint8), t(f"sfq_q_{tag}_1"))
    q0, _ = hpc.scaled_fp8_quant(x, torch.full((), 1e-2, device="cuda"))
    d = (q0.cpu().view(torch.uint8).int() - t(f"sfq_q_{tag}_0").int()).abs()
    assert d.max() <= 1 and (d != 0).float().mean() < 2e-3


@pytest.mark.parametrize("tag", ["a", "b"])
def test_oracle_attention_bf16_matches_reference_output(tag):
    from oracle import attention as oattn

    sq, lens = int(G[f"attn_bf16_{tag}_sq"]), t(f"attn_bf16_{tag}_lens")
    out = oattn.ref_attn_with_paged_kvcache(bf(f"attn_bf16_{tag}_q"), bf(f"attn_bf16_{tag}_kv"),
                                            t(f"attn_bf16_{tag}_bid"), _nblocks(lens, sq), sq, lens)
    assert torch.equal(out, bf(f"attn_bf16_{tag}_out"))


def test_oracle_attention_fp8_matches_reference_output():
    from oracle import attention as oattn

    lens = t("attn_fp8t_lens")
    out = oattn.ref_attn_fp8(f8("attn_fp8t_q"), f8("attn_fp8t_kv"), t("attn_fp8t_bid"), _nblocks(lens, 1), 1, lens,
                             t("attn_fp8t_qs"), torch.tensor([0.7]), torch.tensor([-1.3]), False)
    assert torch.equal(out, bf("attn_fp8t_out"))
    lens = t("attn_fp8k_lens")
    kv = f8("attn_fp8k_kv")
    out = oattn.ref_attn_fp8(f8("attn_fp8k_q"), kv[:, :, :64], t("attn_fp8k_bid"), _nblocks(lens, 2), 2, lens,
                             t("attn_fp8k_qs"), kv[:, 0, 64:], t("attn_fp8k_vs"), True, literal_qscale_row=True)
    assert torch.equal(out, bf("attn_fp8k_out"))


def _moe_inputs():
    rank, E, el = (int(v) for v in G["moe_meta"])
    return (f8("moe_x"), t("moe_xs"), f8("moe_guw"), t("moe_guws"), f8("moe_dw"), t("moe_dws"), t("moe_ids"),
            t("moe_sc"), bf("moe_so")), rank, E


def test_oracle_moe_matches_reference_output():
    from oracle import fuse_moe as omoe

    (x, xs, guw, guws, dw, dws, ids, sc, so), rank, E = _moe_inputs()
    y, inter = omoe.fuse_moe_blockwise_fp8(x, xs, guw, guws, dw, dws, ids, sc, rank, E, so, return_intermediates=True)
    assert torch.equal(inter["topk_pos"], t("moe_topk_pos"))  # routing: bit-exact
    assert allclose(bf("moe_out").float(), y.float(), rtol=2e-3, atol=2e-3)


# ---------------------------------------------------------------------------- GPU: HIP path vs golden
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["a", "b"])
def test_hip_attention_bf16_vs_reference_golden(tag):
    import hpc

    sq, lens = int(G[f"attn_bf16_{tag}_sq"]), t(f"attn_bf16_{tag}_lens")
    kv = bf(f"attn_bf16_{tag}_kv").cuda()
    y = hpc.attention_decode_bf16(bf(f"attn_bf16_{tag}_q").cuda(), kv[:, 0], kv[:, 1], t(f"attn_bf16_{tag}_bid").cuda(),
                                  lens.cuda(), mtp=sq - 1, new_kv_included=False)
    assert allclose(bf(f"attn_bf16_{tag}_out"), y.cpu(), atol=0.016)


@pytest.mark.gpu
def test_hip_attention_fp8_vs_reference_golden():
    import hpc

    lens, kv = t("attn_fp8t_lens"), f8("attn_fp8t_kv").cuda()
    y = hpc.attention_decode_fp8(f8("attn_fp8t_q").cuda(), kv[:, 0], kv[:, 1], t("attn_fp8t_bid").cuda(), lens.cuda(),
                                 t("attn_fp8t_qs").cuda(), torch.tensor([0.7]).cuda(), torch.tensor([-1.3]).cuda(),
                                 mtp=0, new_kv_included=False)
    assert allclose(bf("attn_fp8t_out"), y.cpu(), atol=0.2)
    lens, kv = t("attn_fp8k_lens"), f8("attn_fp8k_kv").cuda()
    y = hpc.attention_decode_fp8(f8("attn_fp8k_q").cuda(), kv[:, 0, :64], kv[:, 1, :64], t("attn_fp8k_bid").cuda(),
                                 lens.cuda(), t("attn_fp8k_qs").cuda(), kv[:, 0, 64:], t("attn_fp8k_vs").cuda(), mtp=1,
                                 new_kv_included=False,
                                 quant_type=hpc.QuantType.QPERTOKEN_PERHEAD_KPERTOKEN_PERHEAD_VPERHEAD)
    assert allclose(bf("attn_fp8k_out"), y.cpu(), atol=0.1)


@pytest.mark.gpu
def test_hip_moe_vs_reference_golden():
    import hpc

    args, rank, E = _moe_inputs()
    d = [a.cuda() for a in args]
    y = hpc.fuse_moe_blockwise_fp8(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], rank, E, d[8])
    assert allclose(bf("moe_out").float(), y.cpu().float(), rtol=0.01, atol=0.01)


@pytest.mark.gpu
def test_hip_rmsnorm_vs_reference_golden():
    import hpc

    y = hpc.fused_rmsnorm_with_scale(bf("norm_x").cuda(), bf("norm_w").cuda(), eps=1e-6,
                                     scale=torch.tensor([2.5]).cuda())
    assert allclose(bf("norm_y8"), y.cpu().to(torch.bfloat16), atol=0.15, rtol=0.0125)


# ---------------------------------------------------------------------------- rope + KV store
def _rope_inputs():
    return (bf("rope_kc0"), bf("rope_vc0"), bf("rope_qkv"), t("rope_cs"), t("rope_ns"), t("rope_qi"),
            t("rope_ki"), t("rope_qw"), t("rope_kw"))


@pytest.mark.parametrize("policy", [0, 1, 2])
def test_oracle_rope_matches_reference_output(policy):
    from oracle import rope as orope

    kc, vc, qkv, cs, ns, qi, ki, qw, kw = _rope_inputs()
    q = orope.rope_norm_ref(kc, vc, qkv, cs, ns, qi, ki, qw, kw, policy)
    assert torch.equal(q, bf(f"rope_q_p{policy}"))
    assert torch.equal(kc, bf(f"rope_k_p{policy}")) and torch.equal(vc, bf(f"rope_v_p{policy}"))


@pytest.mark.gpu
@pytest.mark.parametrize("policy", [0, 1, 2])
def test_hip_rope_vs_reference_golden(policy):
    import hpc

    kc, vc, qkv, cs, ns, qi, ki, qw, kw = [a.cuda() for a in _rope_inputs()]
    q = hpc.rope_norm_store_kv(kc, vc, qkv, cs, ns, qi, ki, True, qw if policy else None, kw if policy else None,
                               qk_norm_policy=policy)
    assert allclose(bf(f"rope_q_p{policy}"), q.cpu(), atol=8e-2)
    assert allclose(bf(f"rope_k_p{policy}"), kc.cpu(), atol=8e-2)
    assert torch.equal(bf(f"rope_v_p{policy}"), vc.cpu())
    # beside the reference's bar: one rounding of the float64 statement plus fp32 slack (tests/utils.py::rope_close)
    from rope_cases import close_to_ref64

    kc0, _, qkv0, cs0, ns0, qi0, ki0, qw0, kw0 = _rope_inputs()
    assert close_to_ref64(q.cpu(), kc.cpu(), kc0, qkv0, cs0, ns0, qi0, ki0, qw0, kw0, policy)


# ---------------------------------------------------------------------------- router GEMM
def test_oracle_router_gemm_matches_reference_output():
    from oracle import gemm as ogemm

    wh, wl = ogemm.split_weight(t("rgemm_w"), 1 / 256)
    assert torch.equal(wh, bf("rgemm_wh")) and torch.equal(wl, bf("rgemm_wl"))
    assert torch.equal(ogemm.ground_truth(bf("rgemm_x"), t("rgemm_w")), t("rgemm_gt"))
    assert allclose(t("rgemm_gt"), ogemm.two_plane(bf("rgemm_x"), wh, wl, 1 / 256), rtol=0.08, atol=0.01)


@pytest.mark.gpu
@pytest.mark.parametrize("fp32_out", [True, False])
def test_hip_router_gemm_vs_reference_golden(fp32_out):
    import hpc

    y = hpc.gemm_bf16xfp32(bf("rgemm_x").cuda(), bf("rgemm_wh").cuda(), bf("rgemm_wl").cuda(), 1 / 256, fp32_out)
    assert allclose(t("rgemm_gt"), y.float().cpu(), rtol=0.08, atol=0.01)


# ---------------------------------------------------------------------------- fused sampler
_SAMP_CFGS = [
    dict(),
    dict(softmax_policy=1, topk=20, topp=0.9),
    dict(softmax_policy=2, topk=50, topp=0.9, max_topk=64),
    dict(softmax_policy=2, topk=torch.tensor([3, 20, 32]), topp=torch.tensor([0.5, 0.9, 0.2]), temperature=0.7,
         repetition_penalty=1.05, with_mask=True),
]


@pytest.mark.parametrize("i", range(4))
def test_oracle_sampler_matches_reference_output(i):
    from oracle import sampler as osamp

    cfg = dict(_SAMP_CFGS[i])
    if cfg.pop("with_mask", False):
        cfg.update(penalty_mask=t("samp_pen"), slot_id=t("samp_slot"))
    tok, pen = osamp.ref_fused_sampler(t("samp_logits"), gumbel_noise=t("samp_gumbel"), **cfg)
    assert torch.equal(tok, t(f"samp_tok_{i}"))
    if pen is not None:
        assert torch.equal(pen, t(f"samp_pen_{i}"))
    if i == 0:
        assert torch.equal(osamp.ref_temperature_sample(t("samp_logits"), t("samp_temp"), t("samp_gumbel")),
                           t("samp_ttok"))
        assert torch.equal(osamp.ref_temperature_sample(t("samp_logits"), t("samp_temp"), t("samp_gumbel"),
                                                        t("samp_draft")), t("samp_ttok_mask"))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(4))
def test_hip_sampler_vs_reference_golden(i):
    import hpc

    cfg = dict(_SAMP_CFGS[i])
    pen = None
    if cfg.pop("with_mask", False):
        pen = t("samp_pen").cuda()
        cfg.update(penalty_mask=pen, slot_id=t("samp_slot").cuda())
    cfg = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in cfg.items()}
    if "topk" in cfg and torch.is_tensor(cfg["topk"]):
        cfg["topk"] = cfg["topk"].to(torch.int64)
    cfg["softmax_policy"] = hpc.SoftmaxPolicy(cfg.get("softmax_policy", 0))
    tok = hpc.fused_sampler(t("samp_logits").cuda(), gumbel_noise=t("samp_gumbel").cuda(), **cfg)
    assert torch.equal(tok.cpu(), t(f"samp_tok_{i}"))
    if pen is not None:
        assert torch.equal(pen.cpu(), t(f"samp_pen_{i}"))
    if i == 0:
        lg, gm = t("samp_logits").cuda(), t("samp_gumbel").cuda()
        assert torch.equal(hpc.fused_sampler(lg, temperature=t("samp_temp").cuda(), gumbel_noise=gm).cpu(), t("samp_ttok"))
        assert torch.equal(hpc.fused_sampler(lg, temperature=t("samp_temp").cuda(), gumbel_noise=gm,
                                             draft_token_ids=t("samp_draft").cuda()).cpu(), t("samp_ttok_mask"))
