"""A plain run of bench.py on the GPU at the smallest size that still has two lockstep groups: it times the steps it was asked for and nothing
else, its line carries ms_per_step, and --dump-outputs holds what the last timed step handed back - the same arrays when the loop runs again."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

SEQUENCES, GROUPS, STEPS, WARMUP = 4, 2, 3, 2


@pytest.mark.gpu
def test_plain_run_times_the_asked_steps_and_dumps_the_last_one(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("PS_SEQ_CACHE", str(tmp_path / "cache"))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    out = tmp_path / "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--sequences", str(SEQUENCES), "--groups", str(GROUPS),
                                      "--distinct", "2", "--scene", "lateral", "--texture", "synthetic", "--dump-outputs", str(out)])
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0
    assert line["metric"] == "tracked frames/sec KITTI stereo 1242x375" and line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    # value = tracked frames of the timed steps / their time: with every frame tracked, sequences x steps over steps x ms_per_step (the line rounds to 5 digits)
    assert line["tracking_checks"]["untracked_frames"] == 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - SEQUENCES) < 1e-3 * SEQUENCES
    for k in ("cpu_baseline", "kernels_alone", "metric_ba", "parity_spot", "config5_one_sequence_per_gpu", "drop_in_api"):      # the legs of --full
        assert k not in line, k
    tcw, fs, ob = (np.load(out / (n + ".npy")) for n in ("tcw", "frame_stats", "object_stats"))
    assert tcw.dtype == np.float32 and tcw.shape == (SEQUENCES, 4, 4) and fs.dtype == np.float64 and fs.shape == (SEQUENCES, 10)
    assert ob.dtype == np.float64 and ob.shape == (SEQUENCES, bench.MAX_OBJECTS, 25)
    assert (fs[:, 1] == 1).all() and np.isfinite(tcw).all() and np.isfinite(ob).all()
    R = tcw[:, :3, :3].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5 and np.array_equal(tcw[:, 3], np.tile(np.float32([0, 0, 0, 1]), (SEQUENCES, 1)))
    assert (ob[..., 0] >= 0).sum() >= SEQUENCES                     # the scene's boxes are in the last frame's records
    # the same loop over the same (cached) sequences again: the dump is the last step of exactly that path, and the path repeats itself
    import torch
    again = bench.tracking_leg(0, 0, "synthetic", STEPS, WARMUP, SEQUENCES, GROUPS, torch.cuda.synchronize, scene="lateral", n_distinct=2)["last_step"]
    assert np.array_equal(again["tcw"], tcw)
    assert np.array_equal(bench._fields_as_float64(again["stats"]), fs) and np.array_equal(bench._fields_as_float64(again["objects"]), ob)
