"""bench.py as the driver runs it: a plain run is the headline only (one JSON line, everything else behind --full), and
--dump-outputs writes what the timed call computed in its last step."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def test_dump_outputs_writes_float32_within_budget(tmp_path):
    """CPU: every tensor becomes <dir>/<name>.npy in float32 with its values; more than the 64 MB budget is refused."""
    sys.path.insert(0, str(ROOT))
    import bench

    y = torch.randn(3, 4, 5).to(torch.bfloat16)
    bench.dump_outputs(tmp_path / "d", {"y": y})
    got = np.load(tmp_path / "d" / "y.npy")
    assert got.dtype == np.float32 and got.shape == (3, 4, 5)
    assert np.array_equal(got, y.float().numpy())
    with pytest.raises(AssertionError):
        bench.dump_outputs(tmp_path / "big", {"z": torch.zeros(1).expand(bench.DUMP_BUDGET_BYTES // 4 + 1)})
    assert not (tmp_path / "big").exists()


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_timed_output(tmp_path):
    """`bench.py --gpus 1 --steps 10 --warmup 2 --dump-outputs DIR`: one JSON line with the headline fields, exactly 10
    timed steps, none of the --full blocks, and DIR/attention_decode_fp8_out.npy equal to the fp8 oracle on the
    regenerated (seeded) inputs for a few requests (reference tolerance atol 0.2)."""
    sys.path.insert(0, str(ROOT))
    import bench
    from oracle import attention as oattn

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["metric"] == "attention_decode_fp8_kv_throughput" and rec["unit"] == "GB/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "fp8_e4m3"
    assert rec["steps"] == 10 and rec["warmup"] == 2 and rec["full"] is False
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    assert rec["parity"] is None and rec["cpu_baseline"] is None and rec["second_metric"] is None and rec["extras"] == {}

    y = np.load(tmp_path / "attention_decode_fp8_out.npy")
    w = bench.C3
    assert y.dtype == np.float32 and y.shape == (w["batch"] * w["num_seq_q"], w["num_head_q"], w["head_dim"])
    assert np.isfinite(y).all() and np.abs(y).max() > 0
    inp = bench.c3_inputs(torch.device("cuda"), dict(w))
    lens = inp["kv_lens"].cpu()
    P = w["block_size"]
    order = torch.argsort(lens).tolist()
    for b in (order[0], order[len(order) // 2], order[-1]):  # shortest, median and longest request
        nb = (int(lens[b]) + P - 1) // P
        ids = inp["block_ids"][b, :nb].long()
        ref = oattn.ref_attn_fp8_separate(inp["q"][b: b + 1].cpu(), inp["k_cache"][ids].cpu(), inp["v_cache"][ids].cpu(),
                                          torch.arange(nb, dtype=torch.int32)[None], lens[b: b + 1], w["num_seq_q"],
                                          inp["q_scale"][b: b + 1].cpu(), inp["k_scale"].cpu(), inp["v_scale"].cpu())
        err = float(np.abs(y[b] - ref.reshape(y[b].shape).float().numpy()).max())
        assert err <= 0.2, (b, err)
