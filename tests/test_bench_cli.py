"""bench.py's command line on the CPU: what a plain run leaves out, what --full keeps, and the --dump-outputs file."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

LEG_SWITCHES = ("no_cpu_baseline", "no_stages", "no_roofline", "no_sd3", "no_parity", "no_cached_mix", "no_two_model")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_times_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "2", "--steps", "7", "--warmup", "2")
    assert not a.full and a.steps == 7 and a.warmup == 2 and a.dump_outputs is None
    assert a.stream_requests == 0 and a.mix == 0 and a.pp == 0
    assert all(getattr(a, s) for s in LEG_SWITCHES)


def test_full_keeps_every_leg(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "2", "--full")
    assert a.stream_requests == 80 and a.mix == 28 and a.pp == 2
    assert not any(getattr(a, s) for s in LEG_SWITCHES)
    a = _parse(monkeypatch, "--full", "--no-sd3", "--mix", "0")
    assert a.no_sd3 and a.mix == 0 and not a.no_roofline


class _Req:
    def __init__(self, seed):
        self.latents = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)


def test_dump_outputs_writes_the_batch_latents_as_fp32(tmp_path):
    reqs = [_Req(i) for i in range(3)]
    bench.dump_outputs(reqs, str(tmp_path / "out"))
    got = np.load(tmp_path / "out" / "latents.npy")
    assert got.dtype == np.float32 and got.shape == (3, 4, 8, 8)
    assert np.array_equal(got, torch.cat([r.latents for r in reqs]).float().numpy())


def test_dump_outputs_past_the_cap_keeps_a_fixed_choice_of_whole_requests(tmp_path, monkeypatch):
    per_req = 4 * 8 * 8 * 4
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 2 * per_req)
    reqs = [_Req(i) for i in range(5)]
    bench.dump_outputs(reqs, str(tmp_path / "a"))
    bench.dump_outputs(reqs, str(tmp_path / "b"))
    a, b = np.load(tmp_path / "a" / "latents.npy"), np.load(tmp_path / "b" / "latents.npy")
    assert a.shape == (2, 4, 8, 8) and a.nbytes <= bench.DUMP_BYTES_MAX and np.array_equal(a, b)
    rows = [next(i for i, r in enumerate(reqs) if np.array_equal(r.latents.float().numpy()[0], x)) for x in a]
    assert rows == sorted(rows) and len(set(rows)) == 2
