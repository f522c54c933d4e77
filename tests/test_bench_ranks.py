"""`bench.py --gpus 2` end to end on the CPU: the real launcher (launch_ranks ->
torch.distributed.run -> one bench.py process per rank), the gloo bootstrap,
ShardedFrame's asynchronous passes with a gather after each, max-over-ranks
timing and rank 0's gather check, with each rank's context replaced by the
oracle-backed stand-in (tests/_bench_standin.py, bench.py --ctx-factory).  The
RCCL transport itself needs >= 2 GPUs (tests/test_multigpu.py).  Those legs run
with --full; the plain run (headline figure only) and --dump-outputs are tested
with the same stand-in and, marked gpu, through libkirk_hip.so."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--full", "--config", "1", "--width", "40", "--height", "24", "--spp", "1", "--depth", "3", "--tile", "8",
        "--steps", "3", "--warmup", "1", "--sync-check-steps", "1", "--iso-steps", "1", "--gui-steps", "0",
        "--ctx-factory", "tests/_bench_standin.py:OracleBenchCtx", "--launch-timeout", "240"]


def _run(gpus, env_extra=None):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), *ARGS], cwd=ROOT,
                          env=env, capture_output=True, text=True, timeout=300)


def _line(stdout):
    return json.loads([ln for ln in stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("gpus", [2, 3])
def test_bench_gpus_n_orchestration(gpus):
    r = _run(gpus)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _line(r.stdout)
    assert line["n_gpus"] == gpus and line["value"] > 0 and line["steps"] == 3
    assert line["config"]["ctx_factory"].endswith("OracleBenchCtx") and line["data"].startswith("STAND-IN")
    chk = line["gather_check"]
    # warmup + instrumented pass + timed + (series start + sync-check) + isolated passes, all gathered
    assert chk["passes"] == 1 + 1 + 3 + (1 + 1) + 1 and chk["pixels"] == 40 * 24
    assert chk["bit_exact"] and chk["mismatched_pixels"] == 0


def test_plain_run_is_lean_and_dumps_the_timed_frame(tmp_path):
    """Without --full the line keeps the headline fields and runs none of the other
    legs; --dump-outputs writes the frame of the warmup + timed passes (here the
    stand-in's, i.e. the oracle's frame of samples 0..3), the same in every run."""
    import numpy as np
    import oracle_ffi
    from _util import assert_parity
    from ba_pathtracing_fur_amd import scenes

    plain =[a for a in ARGS if a != "--full"]
    frames = []
    for d in ("a", "b"):
        env = dict(os.environ, OMP_NUM_THREADS="1")
        env.pop("WORLD_SIZE", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *plain, "--dump-outputs",
                            str(tmp_path / d)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        line = _line(r.stdout)
        assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 1
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "Msamples/s"
        assert line["higher_is_better"] is True and line["dtype"] == "f32"
        for leg in ("roofline", "isolated", "sync_steps", "gui_steps", "gather_check"):
            assert line[leg] is None
        assert "cpu_baseline" not in line and "output_stage" not in line
        assert line["dump_outputs"]["files"] == {"framebuffer.npy": [24, 40, 3],
                                                 "framebuffer_nonfinite.npy": [24, 40, 3]}
        assert line["dump_outputs"]["sampled_pixels"] is None
        frames.append(_dumped_frame(tmp_path / d, (24, 40, 3)))
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))
    want = oracle_ffi.Oracle(scenes.build_config("config1", width=40, height=24)).render(40, 24, 4, 3, threads=2)
    assert_parity(frames[0], want, exact=True)


def _dumped_frame(d, shape):
    """The frame a --dump-outputs directory holds: both files float32, finite and of
    `shape`; the values framebuffer_nonfinite.npy marks are 0 in framebuffer.npy and
    come back here as +inf (1), -inf (2) and NaN (3)."""
    import numpy as np
    assert sorted(os.listdir(d)) == ["framebuffer.npy", "framebuffer_nonfinite.npy"]
    fb, kind = np.load(os.path.join(d, "framebuffer.npy")), np.load(os.path.join(d, "framebuffer_nonfinite.npy"))
    for a in (fb, kind):
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all()
    assert np.isin(kind, (0.0, 1.0, 2.0, 3.0)).all() and not fb[kind != 0].any()
    out = fb.copy()
    for code, v in ((1.0, np.inf), (2.0, -np.inf), (3.0, np.nan)):
        out[kind == code] = v
    return out


@pytest.mark.gpu
def test_plain_run_on_the_gpu_dumps_the_oracles_frame(tmp_path):
    """The plain run through libkirk_hip.so: 1 warmup + 3 timed fused passes of 2 spp
    on a small hairball leave samples 0..7 in the frame, which --dump-outputs
    writes as finite arrays; put together again it must be the oracle's frame
    (inf and NaN by position)."""
    import numpy as np
    import oracle_ffi
    from _util import assert_parity
    from ba_pathtracing_fur_amd import scenes

    W, H = 72, 40
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "2", "--strands", "700",
                        "--width", str(W), "--height", str(H), "--spp", "2", "--depth", "4", "--steps", "3", "--warmup",
                        "1", "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _line(r.stdout)
    assert line["full"] is False and line["n_gpus"] == 1 and line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["roofline"] is None and line["sync_steps"] is None and "cpu_baseline" not in line
    assert not line["data"].startswith("STAND-IN")
    want = oracle_ffi.Oracle(scenes.build_config("config2", width=W, height=H, n_strands=700)).render(W, H, 8, 4, threads=8)
    assert_parity(_dumped_frame(tmp_path, (H, W, 3)), want, exact=True)


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_dump", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_finite_arrays(tmp_path):
    """inf and NaN values of the frame (either NaN encoding) are written as 0 and
    marked 1 (+inf), 2 (-inf), 3 (NaN) in framebuffer_nonfinite.npy; every other
    value is written bit for bit."""
    import numpy as np
    bench = _bench_module()
    fb = np.linspace(-2.0, 5.0, 6 * 5 * 3, dtype=np.float32).reshape(6, 5, 3)
    fb[0, 0, 0], fb[1, 2, 1], fb[5, 4, 2], fb[3, 3, 0] = np.inf, -np.inf, np.nan, -0.0
    fb.view(np.uint32)[2, 1, 2] = 0xFFC00000   # the NaN an invalid operation gives on x86 (0x7FC00000 on gfx950)
    what = bench.dump_outputs(str(tmp_path), fb)
    assert what["nonfinite_values"] == 4 and what["sampled_pixels"] is None and what["bytes"] == 2 * fb.nbytes
    kind = np.load(tmp_path / "framebuffer_nonfinite.npy")
    assert (kind[0, 0, 0], kind[1, 2, 1], kind[5, 4, 2], kind[2, 1, 2]) == (1.0, 2.0, 3.0, 3.0) and (kind != 0).sum() == 4
    got = _dumped_frame(tmp_path, (6, 5, 3))
    fin = np.isfinite(fb)
    assert np.array_equal(got.view(np.uint32)[fin], fb.view(np.uint32)[fin])
    assert np.array_equal(np.isnan(got), np.isnan(fb)) and np.array_equal(got[~fin & ~np.isnan(fb)], fb[~fin & ~np.isnan(fb)])


def test_dump_outputs_samples_a_large_frame(tmp_path):
    """A frame above bench.DUMP_MAX_BYTES is written as a fixed sample of its pixels."""
    import numpy as np
    bench = _bench_module()
    fb = np.arange(50 * 30 * 3, dtype=np.float32).reshape(30, 50, 3)
    fb[7, 7, 1] = np.nan
    assert bench.DUMP_MAX_BYTES <= 64_000_000
    bench.DUMP_MAX_BYTES = 24 * 100
    a = bench.dump_outputs(str(tmp_path / "a"), fb)
    b = bench.dump_outputs(str(tmp_path / "b"), fb)
    assert a == b and a["sampled_pixels"] == 100 and a["bytes"] == 2400
    got = _dumped_frame(tmp_path / "a", (100, 3))
    assert_same = lambda x, y: np.array_equal(x, y, equal_nan=True)
    assert assert_same(got, _dumped_frame(tmp_path / "b", (100, 3)))
    idx = (got[:, 0] / 3).astype(int)   # pixel i holds (3i, 3i+1, 3i+2)
    assert np.all(np.diff(idx) > 0) and assert_same(got, fb.reshape(-1, 3)[idx])


def test_bench_gather_check_fails_loudly():
    """A sender whose pixels arrive altered: the line reports the mismatch and the
    bench exits non-zero (status 3 from the rank, passed on by the launcher)."""
    r = _run(2, {"KHP_STANDIN_CORRUPT": "1"})
    assert r.returncode != 0
    line = _line(r.stdout)
    assert line["gather_check"]["bit_exact"] is False and line["gather_check"]["mismatched_pixels"] > 0
    assert "MISMATCH" in r.stderr


def test_launcher_timeout_kills_the_ranks(tmp_path):
    """launch_ranks: ranks that outlive --launch-timeout are killed, status 124."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_lt", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    stamp = tmp_path / "alive"
    script = tmp_path / "sleeper.py"
    script.write_text(f"import time, pathlib\npathlib.Path({str(stamp)!r}).write_text('x')\ntime.sleep(120)\n")

    class A:
        gpus, launch_timeout = 2, 20.0
    old = sys.argv
    sys.argv = [str(script)]
    try:
        bench.__file__ = str(script)   # the launcher starts this file per rank
        rc = bench.launch_ranks(A())
    finally:
        sys.argv = old
    assert rc == 124 and stamp.exists()
