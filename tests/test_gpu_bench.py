"""bench.py's plain run on the GPU: the result line carries the headline figure only, --steps sets the number of timed
steps, and --dump-outputs writes the state the last timed step left (needs an MI355X). One in-process run of 2 timed
steps after 1 warm-up step on a batch of 4 pairs at 96x128 serves every check."""

import contextlib
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import bench  # noqa: E402

pytestmark = pytest.mark.gpu

FULL_ONLY = ("clock", "roofline", "gemm_kernels", "encoder_conv_roofline", "epe", "infer_960x720", "cpu_baseline")


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    argv = ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4", "--height", "96", "--width",
            "128", "--dump-outputs", str(out)]
    mp = pytest.MonkeyPatch()
    mp.setattr(sys, "argv", argv)
    mp.delenv("WORLD_SIZE", raising=False)
    steps = []
    import stereo_depth_estimation_amd.train as T

    real = T.train_step
    mp.setattr(T, "train_step", lambda *a, **k: (steps.append(1), real(*a, **k))[1])
    import torch

    stdout = io.StringIO()
    try:
        with torch.random.fork_rng(devices=[0]), contextlib.redirect_stdout(stdout):  # main() seeds the generators
            bench.main()
    finally:
        mp.undo()
    return json.loads(stdout.getvalue().strip().splitlines()[-1]), out, len(steps)


def test_plain_result_line_has_the_headline_and_nothing_that_needs_its_own_runs(plain_run):
    line, _, n_steps = plain_run
    assert n_steps == 3  # 1 warm-up + 2 timed: no second region, no EPE training
    assert line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "pairs/s" and line["dtype"] == "bf16"
    assert line["higher_is_better"] is True and line["metric"] == bench.METRIC
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 4 * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]  # 4 pairs per step
    assert not [k for k in FULL_ONLY if k in line]


def test_dump_outputs_writes_the_last_steps_state(plain_run):
    _, out, _ = plain_run
    files = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert set(files) == {"params", "grads", "metrics", "bn_running_mean", "bn_running_var"}
    assert sum(a.nbytes for a in files.values()) <= bench.DUMP_LIMIT_BYTES
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert files["params"].shape == files["grads"].shape == (7_763_938,)  # every trainable element of the base-32 net
    assert files["bn_running_mean"].shape == files["bn_running_var"].shape
    assert all(np.isfinite(a).all() for a in files.values())
    assert np.abs(files["grads"]).max() > 0 and (files["bn_running_var"] > 0).all()
    assert files["metrics"][4] > 0  # valid pixels counted over the 3 steps
