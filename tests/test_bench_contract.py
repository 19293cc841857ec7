"""bench.py / __graft_entry__ contract checks.

CPU: the one-line JSON contract is documented in bench.py and the entry module exposes build() and smoke().
GPU: a short bench run (single-rank path and the multi-rank code path forced on one rank) prints ONE JSON line with
the required keys, a live roofline object for a hot-path kernel and no CPU fallback; smoke() passes.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"]


def test_entry_points_exist():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    assert callable(g.build) and callable(g.smoke)
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in REQUIRED:
        assert '"%s"' % key in src, key
    assert 'json.load(f)["metric"]' in src and "BASELINE.json" in src     # the line carries BASELINE.json's metric verbatim


def test_bench_refuses_experiment_variables():
    """A run with a swapped kernel library or dispatch knobs must not pass for the shipped configuration: exit code 2
    before anything touches a GPU, unless --allow-experiments (the line then records them under env_overrides)."""
    for var in ("ZS_K3_JC", "ZS_HIP_LIBRARY", "ZS_ADAM_GRID"):
        env = dict(os.environ, **{var: "1"})
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1"], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--allow-experiments" in r.stderr and var in r.stderr, (r.returncode, r.stderr[-500:])
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert '"library": library_record(klib)' in src and '"env_overrides": env_overrides()' in src


def test_shipped_library_reads_no_environment():
    """The release build of libzs_hip.so has no getenv: its dispatch depends on call arguments only."""
    import ctypes
    from zhusuan import _hip
    k = _hip.KernelLibrary(_hip.LIB_PATH)
    assert "release (no environment knobs)" in k.build_info()
    out = subprocess.run(["nm", "-D", "--undefined-only", _hip.LIB_PATH], capture_output=True, text=True).stdout
    assert "getenv" not in out, "libzs_hip.so imports getenv: built with -DZS_EXPERIMENTS?"


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return str(sk.getsockname()[1])


def _run_bench(*extra, full=False, env=None):
    """A `--full` run of 6 steps; `full`: return the full record as well."""
    env = dict(os.environ if env is None else env)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    env.setdefault("MASTER_PORT", "29533")
    full_path = os.path.join(tempfile.mkdtemp(prefix="zs_bench_"), "bench_full_test.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "3", "--full", "--full-record", full_path]
                       + list(extra), cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    # (a C++ error prints its message ahead of a long backtrace: keep the lines that name it, not only the tail)
    named = [l for l in r.stderr.splitlines() if "rror" in l or "what()" in l or "terminate" in l or l.startswith("bench:")]
    assert r.returncode == 0, ("\n".join(named)[-3000:], (r.stdout + r.stderr)[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    assert len(lines[0]) <= 8192, "the one-line record must stay under 8 KB (the driver keeps a tail of stdout): %d" % len(lines[0])
    rec = json.loads(lines[0])
    if full:
        return rec, json.load(open(full_path))
    return rec


def test_record_is_flat_where_the_driver_reads_it():
    """The driver keeps the SCALARS of `roofline` (nested dicts do not survive into its parsed record): the fractions the
    contract names are flat keys, and the bulky tables go to the full record, not into the line (VERDICT r03 missing 4)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in ("k1_frac_1M", "k1_frac_4M", "hbm_resident_frac", "k3_fwd_frac"):
        assert 'roof["%s"]' % key in src or '"%s"' % key in src, key
    assert "print(fit_line(out), flush=True)" in src and "LINE_LIMIT = 8192" in src and '"full_record"' in src
    assert 'out["hip_kernels"]' not in src and '"hip_kernels": per_kernel' in src          # per-kernel table: full record only


def _bench_module():
    sys.path.insert(0, ROOT)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        import bench
    finally:
        sys.argv = argv
    return bench


def test_line_is_always_printed_and_always_fits():
    """the 8 KB limit used to be an assertion AFTER all measurements -- a cascade of failing extras (each with an
    unbounded repr) threw the whole record away.  Now: error texts are cut when recorded, and a line that is still too long
    sheds optional parts (failed extras first) and says which."""
    bench = _bench_module()
    base = {"metric": "m", "value": 1.0, "unit": "u", "n_gpus": 1, "steps": 1, "warmup": 0, "ms_per_step": 1.0, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "config": {"workload": "w"},
            "roofline": {"frac": 0.5}, "cpu_baseline": {"value": 1.0}, "library": {"path": "p"}, "env_overrides": {}}
    small = dict(base, extra_configs={"a": {"ms_per_step": 1.0, "value": 2.0}})
    assert json.loads(bench.fit_line(small)) == small                        # nothing touched when it fits
    ex = dict(("ok%d" % i, {"ms_per_step": 1.0, "value": 2.0}) for i in range(10))
    ex.update(("bad%d" % i, {"error": "HIP out of memory " + "x" * 140}) for i in range(80))
    line = bench.fit_line(dict(base, extra_configs=ex))
    assert len(line) <= bench.LINE_LIMIT
    rec = json.loads(line)
    for key in REQUIRED:
        assert key in rec, key
    assert all(("ok%d" % i) in rec["extra_configs"] for i in range(10))      # the measured extras survive, failed ones go first
    assert rec["dropped_from_line"] and all(d.startswith("extra_configs.bad") for d in rec["dropped_from_line"])
    huge = dict(base, config={"workload": "w" * 20000})
    rec = json.loads(bench.fit_line(huge))
    assert len(json.dumps(rec)) <= bench.LINE_LIMIT and rec["metric"] == "m" and rec["value"] == 1.0
    e = RuntimeError("y" * 5000)
    assert len(bench.short(e)) <= 150


def test_ranks_get_the_ipc_setting_and_a_bounded_rendezvous():
    """VERDICT r04 item 1 (b, c): every rank process -- also one started by the driver's own torch.distributed.run -- sets
    HSA_ENABLE_IPC_MODE_LEGACY=0 before torch is imported; the process group has a timeout; a failure exits with one line."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert src.index('os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")') < src.index("import torch")
    assert src.index('os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")') < src.index("def launch_ranks")
    assert 'init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(seconds=COLLECTIVE_TIMEOUT_S))' in src
    assert "os.exec" not in src and "execv" not in src
    env = {k: v for k, v in os.environ.items() if k != "HSA_ENABLE_IPC_MODE_LEGACY"}
    r = subprocess.run([sys.executable, "-c", "import sys, os; sys.argv=['bench.py']; sys.path.insert(0, %r); import bench; "
                        "print(os.environ['HSA_ENABLE_IPC_MODE_LEGACY'])" % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("0"), r.stdout + r.stderr


def test_watchdog_ends_a_stuck_rank_with_one_line():
    code = ("import sys, time; sys.argv=['bench.py']; sys.path.insert(0, %r); import bench\n"
            "w = bench.Watchdog(3, 2.0); w.kick('waiting for a peer'); time.sleep(30)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 5, (r.returncode, r.stderr[-500:])
    assert "rank 3 made no progress" in r.stderr and "waiting for a peer" in r.stderr


@pytest.mark.gpu
def test_bench_line_single_rank():
    rec, full = _run_bench(full=True)
    for key in REQUIRED:
        assert key in rec, key
    cpu = rec["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["sample"] and cpu["one_thread_value"] > 0
    assert rec["n_gpus"] == 1 and rec["steps"] == 6 and rec["warmup"] == 3
    assert rec["higher_is_better"] is True and rec["scaling"] == "weak" and rec["vs_baseline"] is None
    assert rec["dtype"] == "f32" or rec["dtype"] == "fp32"
    assert rec["value"] > 1e5 and abs(rec["value"] - 256 * 50 / (rec["ms_per_step"] * 1e-3)) < 1e-3 * rec["value"]
    roof = rec["roofline"]
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0
    assert 0.05 < roof["frac"] <= 1.0 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-6
    assert all(not isinstance(v, (dict, list)) for v in roof.values()), "roofline must hold scalars only"
    assert "workload" in rec["config"] and "model" not in rec["config"] and "test_mode" not in rec
    assert rec["metric"] == json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
    # --steps is the number of timed steps: one window of exactly 6
    assert rec["trials"] == 1 and abs(1e3 * rec["timed_seconds_total"] - 6 * rec["ms_per_step"]) < 1e-6
    # the north-star kernel's own fraction (beyond the cache), the forward Bernoulli stream and the HBM-resident backward: flat
    for key in ("k1_frac_1M", "k1_frac_4M", "k1_frac_1M_cold", "k1_frac_4M_cold", "hbm_resident_frac", "k3_fwd_frac", "iw1_fwd_frac"):
        assert 0.2 < roof[key] <= 1.0, (key, roof.get(key))
    # THE HEADLINE IS THE PACKAGE DEFAULT: both draws of every latent executed, as the reference does
    assert rec["config"]["discarded_draws"].startswith("executed") and "c3_skip_discarded_draws" in rec["extra_configs"]
    assert rec["config"]["dense_layers"].startswith("zhusuan.Linear in zhusuan.Sequential")
    # the step's generator side is ONE launch each way (IW1): its backward is the kernel that moves the most bytes
    assert rec["config"]["bernoulli_path"].startswith("probs") and roof["kernel"] == "zs_bernoulli_iw_objective_bwd_f32"
    hk = full["hip_kernels"]
    assert hk["zs_bernoulli_iw_objective_f32"]["launches_per_step"] == 1 and hk["zs_bernoulli_iw_objective_bwd_f32"]["launches_per_step"] == 1
    # the discarded draw and the used one: both executed, in ONE launch
    assert hk["zs_normal_sample_logprob_pair_f32"]["launches_per_step"] == 1 and "zs_normal_sample_logprob_f32" not in hk
    assert "one launch per draw" in full["extra_configs"]["c3_one_launch_per_draw"]["discarded_draws"]
    for gone in ("zs_bernoulli_logprob_f32", "zs_normal_logprob_f32", "zs_iw_objective_f32", "zs_normal_logprob_bwd_ksum_f32"):
        assert gone not in hk, gone
    ab1 = hk["zs_dense_act_bwd_f32"]            # caller-side layer kernels: bytes of all their launches, from the calls
    assert ab1["launches_per_step"] == 5 and ab1["algorithmic_bytes_per_step"] == 12 * (12800 * (2 * 500 + 784) + 256 * 2 * 500) + 4 * (4 * 500 + 784)
    lib = rec["library"]
    assert lib["abi"] == 15 and len(lib["sha256"]) == 64 and "release" in lib["build"] and lib["default_path"] is True
    assert lib["path"].endswith("lib/libzs_hip.so") and rec["env_overrides"] == {}
    assert full["trial_ms_per_step"]["min"] <= rec["ms_per_step"] <= full["trial_ms_per_step"]["max"]
    # the same kernels on working sets beyond the Infinity Cache, measured in this run (full record)
    hb = full["hbm_resident"]
    for k in ("zs_bernoulli_logprob_f32", "zs_bernoulli_logprob_bwd_f32", "zs_bernoulli_logits_logprob_f32",
              "zs_bernoulli_logits_logprob_bwd_f32", "zs_normal_sample_logprob_f32"):
        assert hb[k]["algorithmic_bytes"] > 256 * 2 ** 20 and 0.2 < hb[k]["frac_of_hbm_peak"] < 1.0
    # the other configs: compact in the line ({ms_per_step, value}), long form in the full record
    ex, fx = rec["extra_configs"], full["extra_configs"]
    for name in ("c2", "c5", "c3_logits", "iwae_default", "bnn_default", "c3_skip_discarded_draws", "c3_torch_linear", "c3_torch_adam",
                 "c3_default_gemm", "c3_reference_example", "c3_reference_example_graphed", "c5_reference_example",
                 "c5_reference_example_graphed", "c3_eager", "c3_eager_torch_linear", "c5_eager", "c3_forward_only", "c3_one_launch_per_draw",
                 "c5_4_steps_per_graph", "c2_4_steps_per_graph", "c3_4_steps_per_graph"):
        assert ex[name]["value"] > 1e4 and ex[name]["ms_per_step"] > 0 and set(ex[name]) <= {"ms_per_step", "value", "cpu_value"}, (name, ex[name])
        assert np.isfinite(fx[name]["final_loss"])
    # the reference example as written: torch.nn modules, torch.optim.Adam(params, lr), default GEMMs, both draws, eager, fresh batches
    r0 = fx["c3_reference_example"]
    assert r0["launch_mode"].startswith("eager") and "torch.nn.Linear" in r0["dense_layers"] and "reference example" in r0["optimizer"]
    assert r0["mlp_gemm_selection"] == "PyTorch default" and r0["discarded_draws"].startswith("executed") and "new minibatch" in r0["minibatch"]
    r1 = fx["c3_reference_example_graphed"]
    assert r1["launch_mode"] == "hipgraph" and "capturable" in r1["optimizer"] and "new minibatch" in r1["minibatch"]
    # (at the IWAE shape the reference example is GPU-bound either way -- default GEMM picks -- so the graph buys nothing there;
    #  the launch-bound BNN example is where it pays: several times faster with nothing but GraphedStep added)
    assert ex["c5_reference_example_graphed"]["ms_per_step"] < 0.5 * ex["c5_reference_example"]["ms_per_step"]
    for name in ("c2", "c5"):
        cb = fx[name]["cpu_baseline"]
        assert cb["value"] > 0 and cb["one_thread"]["cores"] == 1 and cb["one_thread"]["value"] > 0 and ex[name]["cpu_value"] == cb["value"]
    assert "FlatAdam" in rec["config"]["optimizer"] and "torch.optim.Adam" in fx["c3_torch_adam"]["optimizer"]
    assert np.isfinite(rec["final_loss"]) and rec["full_record"]
    assert "4 steps per replay" in fx["c5_4_steps_per_graph"]["launch_mode"] and fx["c5_4_steps_per_graph"]["steps"] % 4 == 0
    # the step in its default multi-rank form on one rank over RCCL (a child process; this one has no process group)
    dp = ex["c3_dp_step_n1"]
    assert rec["collective_library"] is None and dp["collective_library"].startswith("RCCL") and "hipgraph x2" in fx["c3_dp_step_n1"]["launch_mode"]
    assert fx["c3_dp_step_n1"]["collective_path"].startswith("RCCL called directly")
    assert fx["c3_dp_step_n1"]["mlp_gemm_selection"].endswith("the picks of the parent process")      # the same GEMM kernels in both processes
    assert 0.8 < dp["vs_headline"] < 1.1 and 0.85 < dp["same_process_ratio"] < 1.05 and dp["extra_us_per_step"] < 60.0, dp


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_ones_outputs(tmp_path):
    """Without --full a run sets up, warms up, times exactly --steps steps and prints the line: no roofline, extra_configs, CPU
    baseline or full record.  --dump-outputs writes what the last timed step computed; the same arguments give the same arrays."""
    import glob
    dumps = []
    for i in range(2):
        d, full_path = tmp_path / ("out%d" % i), tmp_path / ("full%d.json" % i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "3",
                            "--dump-outputs", str(d), "--full-record", str(full_path)],
                           cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        rec = json.loads(lines[0])
        assert rec["steps"] == 6 and rec["trials"] == 1 and abs(1e3 * rec["timed_seconds_total"] - 6 * rec["ms_per_step"]) < 1e-6
        assert rec["value"] > 1e5 and abs(rec["value"] - 256 * 50 / (rec["ms_per_step"] * 1e-3)) < 1e-3 * rec["value"]
        assert rec["metric"] == json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
        assert rec["unit"] == "ELBO-evals/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
        assert rec["roofline"] is None and "extra_configs" not in rec and "cpu_baseline" not in rec and "full_record" not in rec
        # the GEMM kernels of every run: the committed picks (per-run tuning lets near-ties come out differently)
        assert rec["config"]["mlp_gemm_selection"].endswith("the picks committed in bench_gemm_picks.csv")
        assert "GEMM picks committed with bench.py loaded" in r.stderr, r.stderr[-2000:]
        assert not full_path.exists()
        files = sorted(glob.glob(str(d / "*.npy")))
        arrays = dict((os.path.basename(f)[:-4], np.load(f)) for f in files)
        assert sum(os.path.getsize(f) for f in files) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert float(arrays["loss"]) == rec["final_loss"] and arrays["iw_bound"].shape == (256,)
        params = [k for k in arrays if k.startswith("param.")]
        assert len(params) == 14 and all(("grad." + k[6:]) in arrays for k in params)
        assert all(np.isfinite(a).all() for a in arrays.values())
        dumps.append(arrays)
    assert sorted(dumps[0]) == sorted(dumps[1])
    for k in dumps[0]:
        np.testing.assert_array_equal(dumps[0][k], dumps[1][k], err_msg=k)


@pytest.mark.gpu
def test_bench_line_with_torch_adam():
    """The step with torch's optimizer (as round 1 ran it)."""
    rec = _run_bench("--no-cpu-baseline", "--no-extras", "--torch-adam")
    assert rec["value"] > 1e5 and rec["config"]["optimizer"].startswith("torch.optim.Adam")
    assert rec["config"]["bernoulli_path"].startswith("probs") and rec["roofline"]["kernel"] == "zs_bernoulli_iw_objective_bwd_f32"


@pytest.mark.gpu
def test_bench_line_strong_scaling_on_one_rank():
    """--strong-scaling: config 4's global batch of 2048 split over the ranks (here: all of it on one GPU: eight datapoints per
    workgroup of the persistent IW1 forward -- round 4's kernel stopped at 384 datapoints; its backward beyond 32 768 rows is K3's
    x-reuse backward plus the K-summed log q gradient, two launches)."""
    rec, full = _run_bench("--no-cpu-baseline", "--no-extras", "--strong-scaling", full=True)
    hk = full["hip_kernels"]
    assert hk["zs_bernoulli_iw_objective_f32"]["launches_per_step"] == 1 and "zs_bernoulli_logprob_f32" not in hk and "zs_iw_objective_f32" not in hk
    assert rec["scaling"] == "strong" and rec["config"]["global_batch"] == 2048 and "batch=2048 per GPU" in rec["config"]["workload"]
    assert abs(rec["value"] - 2048 * 50 / (rec["ms_per_step"] * 1e-3)) < 1e-3 * rec["value"] and np.isfinite(rec["final_loss"])
    assert rec["roofline"]["kernel"] == "zs_bernoulli_logprob_bwd_f32" and 0.4 < rec["roofline"]["frac"] < 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--overlap"], ["--no-direct-rccl"]])
def test_bench_line_collective_path_on_one_rank(extra):
    """The multi-rank forms of the step on ONE rank over RCCL (a process group of one): the default -- one flat bucket filled by
    the backward pass, graph A -> all-reduce on the compute stream -> graph B -- , the staged form (--overlap) and the default
    with torch.distributed's all_reduce instead of the job's own communicator.  The run also replays the same model as a single
    graph, alternating: `same_process` is the path's fixed cost."""
    # (a fresh port per case: the cases run seconds apart, and a fixed one was once still taken)
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=_free_port())
    rec = _run_bench("--no-cpu-baseline", "--no-extras", "--force-collective-path", *extra, env=env)
    assert rec["n_gpus"] == 1 and rec["value"] > 1e5 and rec["collective_library"].startswith("RCCL")
    assert ("hipgraph x3" in rec["config"]["launch_mode"]) == (extra == ["--overlap"])
    assert ("hipgraph x2" in rec["config"]["launch_mode"]) == (extra != ["--overlap"])
    assert rec["collective_path"].startswith("torch.distributed" if extra == ["--no-direct-rccl"] else "RCCL called directly")
    sp = rec["same_process"]
    assert sp["trials_each"] >= 9 and sp["single_graph_ms_per_step"] > 0
    assert 0.8 < sp["collective_path_vs_single_graph"] < 1.05          # (6-step trials: a control-flow test; the 200-step line is the measurement)
    if extra == []:          # (6-step trials: graph launches weigh more than in the 200-step line; the bench line is held to 0.97)
        assert sp["extra_us_per_step"] < 60.0, sp


@pytest.mark.gpu
def test_smoke():
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it: the parent (which never loads torch) starts the two
    ranks itself and relays rank 0's line.  Both ranks share GPU 0 over gloo here (one-GPU box)."""
    env = dict(os.environ)
    env["ZS_BENCH_SHARE_DEVICE"] = "1"
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "3",
                        "--no-cpu-baseline", "--no-gemm-tuning"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["n_ranks_seen"] == 2 and "gloo" in rec["collective_library"]
    assert abs(rec["value"] - 2 * 256 * 50 / (rec["ms_per_step"] * 1e-3)) < 1e-3 * rec["value"]


def test_bench_parent_does_not_load_torch():
    """The rank-launching parent must not initialise the GPU: it decides before torch is imported."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert src.index("raise SystemExit(launch_ranks(") < src.index("import torch")
    r = subprocess.run([sys.executable, "-c",
                        "import sys, runpy; sys.argv=['bench.py','--gpus','2'];\n"
                        "import subprocess; subprocess.call=lambda *a, **k: (print('torch' in sys.modules), 0)[1]\n"
                        "runpy.run_path(%r, run_name='__main__')" % os.path.join(ROOT, "bench.py")],
                       cwd=ROOT, capture_output=True, text=True, timeout=120,
                       env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert r.returncode == 0 and r.stdout.strip().endswith("False"), r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--overlap"], ["--no-graph", "--overlap-allreduce"]])
def test_bench_two_ranks_sharing_one_gpu_over_gloo(extra):
    """The N = 2 control flow end to end (torch.distributed.run, shards, flat bucket, graph A -> all-reduce -> graph B,
    max-over-ranks timing, rank-0 JSON line) on a one-GPU box: both ranks on GPU 0, gloo instead of RCCL."""
    env = dict(os.environ)
    env["ZS_BENCH_SHARE_DEVICE"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "3", "--full",
           "--no-cpu-baseline", "--no-gemm-tuning"] + extra       # (control-flow tests: no need to tune the callers' GEMMs)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "weak"
    assert rec["n_ranks_seen"] == 2 and "gloo" in rec["collective_library"] and rec["replicas_in_sync"] is True
    # default: two graphs around ONE all-reduce on the compute stream; --overlap: three hipGraphs, the decoder-gradient all-reduce
    # overlapping the encoder's backward; --no-graph --overlap-allreduce: eager launches, buckets leaving from autograd hooks
    assert ("overlapped" in rec["config"]["launch_mode"]) == (extra != [])
    assert ("hipgraph x3" in rec["config"]["launch_mode"]) == (extra == ["--overlap"])
    assert ("hipgraph x2" in rec["config"]["launch_mode"]) == (extra == [])
    assert rec["collective_path"].startswith("torch.distributed")          # (gloo test mode: no RCCL communicator)
    assert "NOT a measurement" in rec["test_mode"]
    assert abs(rec["value"] - 2 * 256 * 50 / (rec["ms_per_step"] * 1e-3)) < 1e-3 * rec["value"]
    assert "graph capture failed" not in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_bench_two_ranks_share_one_gemm_tuning_run():
    """Several ranks, tuned GEMMs (the driver's command line has no --no-gemm-tuning): rank 0 evaluates the objective three times on
    a side stream before anything is captured, the other ranks read its picks after a barrier -- one tuning run for the job, the
    same GEMM kernels on every rank.  (The first version ran that pass on the default stream: capture_end crashed on rank 0.)"""
    env = dict(os.environ)
    env["ZS_BENCH_SHARE_DEVICE"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "3", "--full",
           "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["n_ranks_seen"] == 2 and rec["replicas_in_sync"] is True and np.isfinite(rec["final_loss"])
    assert "one tuning run for the job" in rec["config"]["mlp_gemm_selection"] and "hipgraph x2" in rec["config"]["launch_mode"]
    assert "GEMM picks of another process loaded" in r.stderr          # rank 1 read rank 0's file


@pytest.mark.gpu
def test_bench_eight_ranks_sharing_one_gpu_over_gloo():
    """The driver's N = 8 command line end to end on a one-GPU box: 8 ranks (torch.distributed.run) on GPU 0 over gloo --
    per-rank shards and Philox streams, the flat bucket (two hipGraphs per rank around one eagerly launched collective),
    max-over-ranks timing, ONE JSON line from rank 0 with n_gpus = n_ranks_seen = 8.  A control-flow test
    (RCCL refuses two ranks on one device): no 2 / 4 / 8-GPU NUMBER exists until the driver runs one."""
    env = dict(os.environ)
    env["ZS_BENCH_SHARE_DEVICE"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "6", "--warmup", "3", "--full",
           "--no-cpu-baseline", "--no-gemm-tuning"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 8 and rec["n_ranks_seen"] == 8 and rec["scaling"] == "weak" and "gloo" in rec["collective_library"]
    assert rec["replicas_in_sync"] is True
    assert "hipgraph x2" in rec["config"]["launch_mode"] and rec["config"]["global_batch"] == 2048
    assert "dp8" in rec["config"]["parallelism"] and "one flat bucket" in rec["config"]["parallelism"]
    assert abs(rec["value"] - 8 * 256 * 50 / (rec["ms_per_step"] * 1e-3)) < 1e-3 * rec["value"]
    assert "NOT a measurement" in rec["test_mode"] and np.isfinite(rec["final_loss"])
    assert "graph capture failed" not in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--overlap"]])
def test_one_ranks_failed_capture_takes_every_rank_to_eager_launches_together(extra):
    """VERDICT r04 item 1 (a, d): rank 1's graph capture is made to fail.  The ranks meet (all-reduce MIN of "capture ok") and
    fall back TOGETHER to the same stages launched eagerly -- the same collectives, so nobody waits for ever and nothing is
    summed into the wrong buffer: the run ends normally, the line says so, and the replicas' parameters are bit-identical."""
    env = dict(os.environ)
    env["ZS_BENCH_SHARE_DEVICE"] = "1"
    env["ZS_BENCH_FAIL_CAPTURE_RANK"] = "1"
    env["ZS_BENCH_WATCHDOG_S"] = "300"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "3", "--full",
           "--no-cpu-baseline", "--no-gemm-tuning"] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_ranks_seen"] == 2 and rec["replicas_in_sync"] is True and np.isfinite(rec["final_loss"])
    assert rec["config"]["launch_mode"].startswith("eager (graph capture failed on a rank; all ranks fell back together)")
    assert ("two staged all-reduces" in rec["config"]["launch_mode"]) == (extra == ["--overlap"])
    assert "capture failure injected on rank 1" in r.stderr          # rank 1 says why
    assert r.stderr.count("gave way to eager launches on every rank") == 2        # ... and BOTH ranks changed mode
    assert rec["env_overrides"].get("ZS_BENCH_FAIL_CAPTURE_RANK") == "1"


@pytest.mark.gpu
def test_a_rank_that_stops_ends_the_job_with_a_reason_instead_of_a_hang():
    """Rank 1 stops making progress before the timed region.  Nobody can look at the node: the run must END, non-zero, with one
    line naming the rank and the stage (the watchdog; under RCCL the process group's timeout does the same for a collective)."""
    import time
    env = dict(os.environ)
    env["ZS_BENCH_SHARE_DEVICE"] = "1"
    env["ZS_BENCH_STALL_RANK"] = "1"
    env["ZS_BENCH_WATCHDOG_S"] = "25"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "3",
           "--no-cpu-baseline", "--no-gemm-tuning"]
    t0 = time.time()
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode != 0
    assert "made no progress" in r.stderr and "giving up, exit code 5" in r.stderr, r.stderr[-2000:]
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]           # no line from a run that did not finish
    assert time.time() - t0 < 600
