"""bench.py's static contract (no GPU): every workload names a registered env and an oracle class, the algorithmic bytes
are SURVEY 8(d)'s figures, and the CPU-baseline leg produces the fields the driver reads."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_workloads_are_consistent(oracle):
    import gym_xarm_amd
    b = _bench()
    assert set(b.WORKLOADS) == {"pnp", "reach", "handover", "stack", "handover2"} == set(b.WORKLOAD_NAMES) == set(b.SUBSTEPS)
    survey_bytes = {"pnp": 452, "reach": 336, "handover": 648, "stack": 1040, "handover2": 836}    # SURVEY.md 8(d) (+ its rule for N = 2)
    default_envs = {"pnp": 65536, "reach": 4096, "handover": 16384, "stack": 8192, "handover2": 16384}     # BASELINE.json configs, per GPU
    for w, (env_id, E, act_dim, nbytes, kernel, cls, sample, cfg) in b.WORKLOADS.items():
        assert env_id in gym_xarm_amd.registered_ids()
        assert hasattr(oracle, cls)
        assert nbytes == survey_bytes[w] and E == default_envs[w]
        assert act_dim == (4 if w in ("pnp", "reach") else 8)
    assert b.HBM_PEAK_GBS == 8000.0


def test_cpu_baseline_leg_reports_the_contract_fields(oracle, monkeypatch):
    b = _bench()
    monkeypatch.setitem(b.WORKLOADS, "reach", b.WORKLOADS["reach"][:6] + ((4, 3),) + b.WORKLOADS["reach"][7:])   # tiny sample
    monkeypatch.setattr(os, "cpu_count", lambda: 2)
    out = b.cpu_baseline("reach")
    assert set(out) >= {"value", "unit", "cores", "kind", "sample"}
    assert out["kind"] == "port" and out["cores"] == 2 and out["value"] > 0 and "XarmReach-v0" in out["sample"]


def test_cpu_baseline_sample_is_what_baseline_md_asks_for(oracle):
    """the oracle over 4 096 envs on all cores; the sample string says how it is threaded"""
    b = _bench()
    for w, row in b.WORKLOADS.items():
        assert row[6][0] == 4096, w
    import inspect
    src = inspect.getsource(b.cpu_baseline)
    assert "not OpenMP" in src and "ThreadPoolExecutor" in src


def test_json_line_carries_the_library_identity_and_refuses_variants(tmp_path):
    """xarm_version() / library path / pipeline / solver constants come from the handle, and a TIMING VARIANT
    or XARM_HIP_LIB without --allow-variant-lib ends the run non-zero (checked on the stand-in env: bench.py's own logic)"""
    import json
    import subprocess
    import sys
    env = dict(os.environ, XARM_BENCH_DEVICE="cpu", XARM_BENCH_ENV_FACTORY="tests.bench_stub:make", PYTHONPATH=ROOT)
    env.pop("XARM_HIP_LIB", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--repeats", "1", "--envs-per-gpu", "8", "--no-extras", "--no-cpu-baseline"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    lib = j["library"]
    assert set(lib) >= {"version", "path", "variant", "pipeline", "reset_coop_limit", "step_coop_limit"} and lib["variant"] is False
    assert j["config"]["solver_iterations"] == 50 == lib["pipeline"]["solver_iterations"]
    assert "avg_ms_is" in j["roofline"]["kernels"]["reset"]
    bad = subprocess.run(cmd, env=dict(env, XARM_HIP_LIB="/nonexistent/lib_variant.so"), capture_output=True, text=True, cwd=ROOT)
    assert bad.returncode != 0 and "not the product build" in bad.stderr
    ok = subprocess.run(cmd + ["--allow-variant-lib"], env=dict(env, XARM_HIP_LIB="/nonexistent/lib_variant.so"), capture_output=True, text=True, cwd=ROOT)
    assert ok.returncode == 0 and json.loads([l for l in ok.stdout.splitlines() if l.startswith("{")][-1])["library"]["variant"] is True


def _stub_run(args, tmp_path):
    import json
    import subprocess
    import sys
    env = dict(os.environ, XARM_BENCH_DEVICE="cpu", XARM_BENCH_ENV_FACTORY="tests.bench_stub:make", PYTHONPATH=ROOT)
    env.pop("XARM_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_plain_run_times_exactly_steps_and_nothing_else(tmp_path):
    """without --full: one window of exactly --steps calls, no extra legs, no CPU baseline; the headline fields as before"""
    j = _stub_run(["--gpus", "1", "--steps", "9", "--warmup", "2", "--envs-per-gpu", "16"], tmp_path)
    assert j["steps"] == 9 and j["warmup"] == 2 and j["repeats"]["n"] == 1 and j["roofline"]["kernel_launches"] == 9
    assert j["metric"].startswith("env steps/sec") and j["unit"] == "env steps/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert abs(j["value"] - 16 * 9 / (j["ms_per_step"] * 9e-3)) < 1e-6 * j["value"]
    assert not {"aged_state", "lockstep_phase", "lazy_reset", "strong_scaling", "cpu_baseline"} & set(j)
    full = _stub_run(["--gpus", "1", "--steps", "9", "--warmup", "2", "--envs-per-gpu", "16", "--full", "--aged-preroll", "5"], tmp_path)
    assert full["repeats"]["n"] == 3 and {"aged_state", "lockstep_phase", "lazy_reset", "cpu_baseline"} <= set(full)


def test_dump_outputs_writes_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: every array the caller of env.step got from the last timed step, float32 / float64, the same
    bytes from run to run"""
    import numpy as np
    runs = []
    for k in range(2):
        d = tmp_path / ("out%d" % k)
        _stub_run(["--steps", "7", "--warmup", "3", "--envs-per-gpu", "12", "--dump-outputs", str(d)], tmp_path)
        runs.append({p.stem: np.load(p) for p in d.glob("*.npy")})
    assert set(runs[0]) == {"reward", "done", "info_is_success", "info_resetting"}
    for k, a in runs[0].items():
        assert a.dtype in (np.float32, np.float64) and a.shape == (12,) and np.array_equal(a, runs[1][k]), k
    # the stand-in's 10-step episodes from desynchronised phases (gid * 7919 % 10): step 3 + 7 ends those that started at phase 0
    assert np.array_equal(runs[0]["done"], (np.arange(12) * 7919 % 10 == 0).astype(np.float32))
    assert np.array_equal(runs[0]["done"], runs[0]["info_is_success"])


def test_dump_outputs_samples_rows_above_the_limit(tmp_path, monkeypatch):
    import numpy as np
    import torch
    b = _bench()
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 4000)
    E = 100
    obs = {"observation": torch.arange(E * 24, dtype=torch.float32).reshape(E, 24)}
    info = {"is_success": torch.ones(E, dtype=torch.uint8), "TimeLimit.truncated": torch.zeros(E, dtype=torch.bool)}
    b.dump_outputs((obs, torch.arange(E, dtype=torch.float32), torch.zeros(E, dtype=torch.uint8), info), str(tmp_path))
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(got) == {"observation", "reward", "done", "info_is_success", "info_TimeLimit_truncated", "sample_rows"}
    assert sum(a.nbytes for a in got.values()) <= 4000
    rows = got["sample_rows"].astype(np.int64)
    assert 0 < rows.size < E and np.array_equal(got["reward"], rows.astype(np.float32))
    assert np.array_equal(got["observation"], obs["observation"].numpy()[rows])
