#!/usr/bin/env python
"""bench.py -- ELBO-evals/s of the variational-inference hot path on MI355X.

Workload (BASELINE.json configs[2] / per-GPU shape of configs[3]): IWAE on MNIST-shaped synthetic bits,
VIMCO estimator, batch 256 per GPU, K = 50 particles, latent 40, x 784, hidden 500, fp32.
One step = objective forward (sampling, log-probs, VIMCO reduction in HIP kernels; MLPs in
hipBLASLt via PyTorch) + backward + [all-reduce of the flat gradient buckets] + Adam.
One ELBO-eval = one log-importance-weight log w[k, b], so a step does B*K evals per GPU.

  python bench.py [--gpus N --steps K --warmup W]          (N > 1: this process only starts the N ranks, see launch_ranks)
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...   (the driver's form for N > 1)

Timing: EXACTLY `--steps` steps in one window, bracketed by torch.cuda.synchronize() + a barrier on both sides and reduced
with MAX over the ranks; `ms_per_step` is that window over `--steps`.

A plain run sets up, warms up (`--warmup` steps), times the steps, writes the last step's outputs (`--dump-outputs DIR`)
and prints the line with the headline figure.  Everything else it can measure or check runs only with `--full`.

Rank 0 prints ONE JSON line (contract in the task description; kept under 8 KB) with, under `--full`,
  `roofline`      the hot-path kernel that moves the most bytes per step (the backward of the Bernoulli stream), timed live
                  in the launch mode of the timed region, plus flat scalars for the other kernels the contract names:
                  `k1_frac_1M`, `k1_frac_4M` (the fused Normal sample + log-prob kernel beyond the cache), `k3_fwd_frac`,
                  `hbm_resident_frac`;
  `cpu_baseline`  the CPU oracle (oracle/zs_oracle.py) on the same workload on this host's cores (calibrated thread
                  count, plus a 1-thread figure);
  `extra_configs` {name: {ms_per_step, value}}: the other single-GPU BASELINE configs, the reference example as written
                  (torch.nn modules, torch.optim.Adam, default GEMM selection, an eager Python loop over fresh minibatches),
                  the same with only GraphedStep added, eager launches of the headline step, the opt-ins;
  `full_record`   the file (bench_full.json next to this script) that holds everything else: per-kernel tables
                  (`hip_kernels`, `hbm_resident`), trial times, the long-form description of every setting.
"""
import argparse
import json
import os
import sys
import time

# dmabuf IPC only on this pool: RCCL (and any CUDA-tensor sharing across processes) fails with "hipIpcGetMemHandle: invalid
# argument" without it.  Set here, before torch is imported, so that a rank started by ANY launcher (the driver's
# `python -m torch.distributed.run ... bench.py --gpus N` as well as launch_ranks below) has it.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "zhusuan-pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCH_PER_GPU, PARTICLES, Z_DIM, X_DIM, HIDDEN = 256, 50, 40, 784, 500
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
DEFAULT_GEMM_PICKS = os.path.join(ROOT, "bench_gemm_picks.csv")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything beyond the headline figure as well: the per-kernel timing passes and the "
                         "roofline, the K1 and HBM-resident kernel figures, extra_configs, the CPU baselines, the same-process twin "
                         "of --force-collective-path, the replica check of several ranks and the full record (--full-record)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last of them computed as DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--fused-logits", action="store_true",
                    help="the decoder hands logits to Bernoulli(logits=...): its final sigmoid is formed inside the log-prob "
                         "kernel instead of a separate pass over [K, B, 784] (extra_configs.c3_logits in the default run; the "
                         "default keeps the nn.Sigmoid pass and Bernoulli(probs=...) of the reference's example)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip extra_configs and the HBM-resident kernel figures")
    ap.add_argument("--force-collective-path", action="store_true",
                    help="run the multi-rank code path (bucket pack + all-reduce + split graphs) even with one rank")
    ap.add_argument("--overlap", action="store_true",
                    help="multi-rank, graphs: the STAGED step -- two buckets, three graphs: the decoder-gradient all-reduce runs on "
                         "the collective library's stream beside the encoder's backward (zhusuan.dataparallel.StagedBuckets).  Not "
                         "the default since round 6: at this model's size the fork / join around the overlapped collective costs "
                         "about what it hides (DESIGN.md section 7, profiles/r06_stream_links.txt)")
    ap.add_argument("--no-direct-rccl", action="store_true",
                    help="all-reduce through torch.distributed (two HIP event records per call) instead of this job's own RCCL "
                         "communicator driven on the compute stream (zhusuan.dataparallel.DirectAllReduce)")
    ap.add_argument("--gemm-picks", default=DEFAULT_GEMM_PICKS,
                    help="a TunableOp results file to start from: its GEMM picks are used as they are, only shapes it lacks are tuned.  "
                         "Default: bench_gemm_picks.csv next to this script (the fastest fp32 solutions for the workloads' shapes, timed "
                         "on an MI355X), so that every run computes with the same GEMM kernels; \"\" times every shape afresh.  The "
                         "parent of the c3_dp_step_n1 child passes its own picks")
    ap.add_argument("--timeline", default="",
                    help="write a chrome trace (torch.profiler: host runtime calls + device activity) of 5 steps in the timed "
                         "region's launch mode to this path (tools/timeline_gaps.py reads it)")
    ap.add_argument("--no-graph", action="store_true",
                    help="launch every kernel from Python each step instead of replaying captured hipGraphs")
    ap.add_argument("--no-overlap", action="store_true",
                    help="(the default since round 6; kept for old command lines) multi-rank, graphs: ONE bucket all-reduced on "
                         "the compute stream after the whole backward: graph A -> all-reduce -> graph B (the update)")
    ap.add_argument("--overlap-allreduce", action="store_true",
                    help="eager launches only (--no-graph): all-reduce gradient buckets from autograd hooks while backward "
                         "is still running (zhusuan.dataparallel.OverlappedBuckets)")
    ap.add_argument("--blas", default="default", choices=["default", "hipblaslt", "rocblas"],
                    help="BLAS library PyTorch uses for the MLPs' fp32 GEMMs (outside the hot path)")
    ap.add_argument("--no-gemm-tuning", action="store_true",
                    help="leave PyTorch's default GEMM solution selection for the callers' fp32 nn.Linear stack (default: PyTorch "
                         "TunableOp picks the fastest fp32 hipBLASLt / rocBLAS solution per GEMM shape during warm-up)")
    ap.add_argument("--allow-experiments", action="store_true",
                    help="run although ZS_* experiment variables are set (ZS_HIP_LIBRARY: another build of the kernel library; "
                         "ZS_K*: dispatch knobs of a -DZS_EXPERIMENTS build) or the loaded library is an experiments build; the "
                         "line then says so (`env_overrides`, `library`).  Without the flag such a run is refused (exit code 2)")
    ap.add_argument("--skip-discarded-draws", action="store_true",
                    help="run the step inside zhusuan.skip_discarded_draws(): the draw of every latent that the reference's "
                         "objectives throw away (the node factory's sample, bn.py:158 / elbo.py:122) is then not executed.  An "
                         "opt-in of the package, OFF by default here as in the package (extra_configs.c3_skip_discarded_draws in "
                         "the default run)")
    ap.add_argument("--reference-draws", action="store_true", help="(default since round 4; kept for old command lines)")
    ap.add_argument("--full-record", default=os.path.join(ROOT, "bench_full.json"),
                    help="where the long-form record of --full goes (per-kernel tables, trial times, setting descriptions)")
    ap.add_argument("--torch-linear", action="store_true",
                    help="build the callers' MLPs from torch.nn.Linear / Sequential (as the reference's examples do) instead of "
                         "zhusuan.Linear / zhusuan.Sequential -- the same layers (parameters, names, GEMMs) with the ReLU in the forward "
                         "GEMM's epilogue and the activation's backward + the bias gradient as ONE deterministic launch (AB1 / CS1) "
                         "instead of torch's clamp, threshold_backward and generic reduction; extra_configs.c3_torch_linear in the "
                         "default run")
    ap.add_argument("--unfused-activations", action="store_true",
                    help="zhusuan.Linear inside torch.nn.Sequential: only the bias gradient is this package's (CS1), the activations "
                         "are torch's passes (round 3's first setting; extra_configs.c3_unfused_activations in the default run)")
    ap.add_argument("--strong-scaling", action="store_true",
                    help="split config 4's GLOBAL batch of 2048 over the ranks (2048 / N datapoints per GPU; N must divide 2048) instead of "
                         "256 per GPU: the line then says \"scaling\": \"strong\" (SURVEY.md 8d: 'also strong scaling B = 2048 total'). "
                         "The default, and what the driver runs, is weak scaling")
    ap.add_argument("--batch-per-gpu", type=int, default=0,
                    help="(kernel studies only, not a BASELINE config: the line's config.workload says so) datapoints per GPU instead of 256")
    ap.add_argument("--iw1-max-stream-bytes", type=int, default=-1,
                    help="(kernel studies only) override zhusuan._ops.IW1_MAX_STREAM_BYTES: 0 = never the fused generator-side launch")
    ap.add_argument("--torch-adam", action="store_true",
                    help="update with torch.optim.Adam(fused=True, capturable=True) instead of zhusuan.optim.FlatAdam "
                         "(the same update over flat buckets, one launch)")
    return ap.parse_args(argv)


def launch_ranks(n_ranks, argv):
    """`python bench.py --gpus N` without a launcher around it: this process becomes the PARENT of N ranks.  It has
    not imported torch or touched the GPU (and never will): it starts `python -m torch.distributed.run` with the
    same arguments as a child process, one rank per GPU over RCCL, relays the child's output (rank 0 prints the one
    JSON line) and exits with its return code.  Nothing is exec'ed."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)                                # (carries HSA_ENABLE_IPC_MODE_LEGACY=0, set at the top of this file)
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    sys.stderr.write("bench: launching %d ranks: %s\n" % (n_ranks, " ".join(cmd)))
    return subprocess.call(cmd, env=env, cwd=ROOT)


# ZS_* variables that are this script's own test hooks (reported, never refused); every other ZS_* variable is an experiment
_BENCH_OWN_ENV = ("ZS_BENCH_SHARE_DEVICE", "ZS_BENCH_NO_TRACER", "ZS_BENCH_FAIL_CAPTURE_RANK", "ZS_BENCH_STALL_RANK",
                  "ZS_BENCH_WATCHDOG_S", "ZS_BENCH_NO_SHARED_PICKS")


def env_overrides():
    """Every ZS_* variable set in this process's environment: the line records them all."""
    return dict((k, v) for k, v in sorted(os.environ.items()) if k.startswith("ZS_"))


def refuse_experiments(args):
    """A number measured with a swapped library or dispatch knobs must not pass for the shipped configuration."""
    bad = [k for k in env_overrides() if k not in _BENCH_OWN_ENV]
    if bad and not args.allow_experiments:
        sys.stderr.write("bench: refusing to run with experiment variables set (%s); unset them or pass --allow-experiments "
                         "(the JSON line then records them)\n" % ", ".join(bad))
        raise SystemExit(2)


if __name__ == "__main__":
    refuse_experiments(parse_args())
if __name__ == "__main__" and "RANK" not in os.environ:
    _a = parse_args()
    if _a.gpus > 1:
        raise SystemExit(launch_ranks(_a.gpus, sys.argv[1:]))

import numpy as np                    # noqa: E402  (after the parent-only branch above: the parent never loads torch)
import torch                          # noqa: E402
import torch.distributed as dist      # noqa: E402


def baseline_metric():
    """BASELINE.json's metric string, verbatim (the K = 50 MNIST workload it is quoted on is the IWAE / VIMCO example:
    config.workload names it)."""
    try:
        with open(os.path.join(ROOT, "BASELINE.json")) as f:
            return json.load(f)["metric"]
    except (OSError, ValueError, KeyError):
        return "ELBO-evals/sec (batch\u00d7K particles) VAE-MNIST K=50 @1/2/4/8 GPU"


GEMM_PICKS = {"loaded_from": None}


def gemm_picks_file(kind="tuned"):
    import tempfile                  # TunableOp writes its picks there: keep that file out of the repository
    return os.path.join(tempfile.gettempdir(), "zs_bench_tunableop_%s%d.csv" % ("" if kind == "tuned" else kind + "_", os.getpid()))


def save_gemm_picks(path):
    """Every TunableOp pick this process holds -- read from a file or tuned here -- as one results file another process can
    start from (TunableOp's own file receives only the shapes tuned in this process)."""
    import torch.cuda.tunable as tunable
    with open(path, "w") as f:
        for key, value in tunable.get_validators():
            f.write("Validator,%s,%s\n" % (key, value))
        for op, params, kernel, duration in tunable.get_results():
            f.write("%s,%s,%s,%s\n" % (op, params, kernel, duration))
    return path


def gemm_tuning(on, tune=True, picks=None):
    """The callers' MLPs (outside the hot path, 72 % of the step) are fp32 GEMMs dispatched by PyTorch.  Its TunableOp
    times the available fp32 hipBLASLt / rocBLAS solutions for each GEMM shape once (during the eager warm-up steps,
    ~4 s in total for this workload) and uses the fastest from then on: same precision, same arithmetic, another tiling.
    `--no-gemm-tuning` measures with PyTorch's default heuristic selection.  `picks`: a results file to start from -- by default
    bench_gemm_picks.csv: near-ties between solutions come out differently from run to run, and the last-bit differences of two
    sets of GEMM kernels grow over a few hundred Adam steps into a different trained state; with the committed picks every run
    computes the same step.  The one-rank child of c3_dp_step_n1 takes its parent's picks: the two processes then run the same
    GEMM kernels, and what is left of `vs_headline` is the step's form.  Shapes the file lacks are tuned as usual."""
    try:
        import torch.cuda.tunable as tunable
        tunable.enable(bool(on))
        tunable.tuning_enable(bool(on and tune))
        if on:
            tunable.set_max_tuning_duration(30)
            tunable.set_filename(gemm_picks_file())
            if picks and os.path.exists(picks):
                try:
                    ok = tunable.read_file(picks)
                    GEMM_PICKS["loaded_from"] = picks if ok else None
                    sys.stderr.write("bench: GEMM picks %s %s (%s)\n" % ("committed with bench.py" if picks == DEFAULT_GEMM_PICKS else
                                                                          "of another process", "loaded" if ok else "NOT loaded", picks))
                except Exception as e:                              # noqa: BLE001
                    sys.stderr.write("bench: could not read the GEMM picks %s (%r); tuning afresh\n" % (picks, e))
        return bool(on)
    except Exception as e:                                          # noqa: BLE001
        sys.stderr.write("bench: TunableOp unavailable (%r); default GEMM selection\n" % (e,))
        return False


def collective_library(share_device):
    if share_device:
        return "gloo (test mode)"
    try:
        return "RCCL %s" % ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception:                                               # noqa: BLE001
        return "RCCL (version unavailable)"


def library_record(klib):
    """Which kernel library produced the numbers: path, content hash, ABI and the library's own build description."""
    import hashlib
    h = hashlib.sha256()
    with open(klib.path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return {"path": os.path.relpath(klib.path, ROOT) if klib.path.startswith(ROOT) else klib.path, "sha256": h.hexdigest(),
            "abi": klib.cdll.zs_abi_version(), "build": klib.build_info(),
            "default_path": os.environ.get("ZS_HIP_LIBRARY") is None}


def pmc_traffic(entry, fused_logits, abi_version):
    """HBM bytes per launch of `entry` from the PMC passes committed under profiles/ (rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE in separate runs of this bench command, gfx950 FETCH_SIZE x2 correction applied).  Counters cannot be
    read from inside this process, so the figure is NOT measured in this run: it is returned with its provenance, and
    only when the profile was taken with the same kernel library ABI and the same Bernoulli path (None otherwise)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))
    if not files:
        return None, None
    try:
        with open(files[-1]) as f:
            doc = json.load(f)
        if doc.get("abi_version") != abi_version or bool(doc.get("fused_logits", False)) != bool(fused_logits):
            return None, {"source": os.path.relpath(files[-1], ROOT), "measured_in_this_run": False,
                          "note": "profile does not match this run (kernel library ABI or Bernoulli path): not reported"}
        k = doc["kernels"].get(entry)
        if not k:
            return None, None
        return k["hbm_bytes_corrected"], {"source": os.path.relpath(files[-1], ROOT), "measured_in_this_run": False,
                                          "tool": doc.get("tool"), "traffic_over_algorithmic": k.get("traffic_over_algorithmic")}
    except (OSError, ValueError, KeyError):
        return None, None


# ------------------------------------------------------------------------------------------------ workloads
def make_workload(name, dev, seed_rank=0, fused_logits=False, dense="fused"):
    """(model, observations, ELBO-evals per step, description) of a BASELINE config on one GPU."""
    from examples import iwae, vae_mnist, bnn_vi
    rs = np.random.RandomState(1234 + seed_rank)
    bits = lambda B: torch.tensor((rs.uniform(size=(B, X_DIM)) < 0.5).astype(np.float32), device=dev)
    if name in ("c3", "c3_logits", "c3_probs"):
        fused = name == "c3_logits" or (fused_logits and name != "c3_probs")
        model = iwae.build(n_samples=PARTICLES, estimator="vimco", x_dim=X_DIM, z_dim=Z_DIM, hidden=HIDDEN, device=dev,
                           fused_logits=fused, dense=dense)
        return model, {"x": bits(BATCH_PER_GPU)}, BATCH_PER_GPU * PARTICLES, \
            "IWAE-MNIST VIMCO, batch=256, K=50, " + ("Bernoulli from logits (the decoder's sigmoid inside the log-prob kernel)"
                                                      if fused else "Bernoulli from probabilities (nn.Sigmoid pass, as the reference's example)")
    if name == "c2":
        return vae_mnist.build(512, device=dev, dense=dense), {"x": bits(512)}, 512, "VAE-MNIST SGVB, batch=512, K=1 (BASELINE configs[1])"
    if name == "c5":
        x = torch.tensor(rs.standard_normal((512, 13)).astype(np.float32), device=dev)
        y = torch.tensor(rs.standard_normal(512).astype(np.float32), device=dev)
        return bnn_vi.build(n_particles=10, device=dev), {"x": x, "y": y}, 5120, \
            "BNN-VI [13,50,1], batch=512 per GPU, K=10 (per-GPU shape of BASELINE configs[4])"
    if name == "iwae_default":      # the reference example's own settings (examples/variational_autoencoder/iwae.py:126,131)
        model = iwae.build(n_samples=40, estimator="vimco", x_dim=X_DIM, z_dim=Z_DIM, hidden=HIDDEN, device=dev, dense=dense)
        return model, {"x": bits(64)}, 64 * 40, "IWAE-MNIST VIMCO, batch=64, K=40 (the reference example's defaults, iwae.py:126,131)"
    if name == "bnn_default":       # examples/bayesian_neural_nets/bnn_vi.py:116-118
        x = torch.tensor(rs.standard_normal((114, 13)).astype(np.float32), device=dev)
        y = torch.tensor(rs.standard_normal(114).astype(np.float32), device=dev)
        return bnn_vi.build(n_particles=512, device=dev), {"x": x, "y": y}, 114 * 512, \
            "BNN-VI [13,50,1], batch=114, K=512 (the reference example's defaults, bnn_vi.py:116-118)"
    raise ValueError(name)


def cpu_model_name():
    """The host CPU's model string (/proc/cpuinfo), as SURVEY.md section 8d asks next to the CPU baseline."""
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.lower().startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine() or "unknown"


def cpu_step_fn(name, optimizer=True):
    """One training step of the CPU oracle on workload `name`: fwd + bwd + Adam, or (optimizer=False) fwd + bwd only -- what
    BASELINE.md's table of the reference on the host cores times.  Returns (step, evals per step)."""
    from oracle import zs_oracle as O
    import helpers as H
    rng = np.random.RandomState(1234)
    if name in ("c3", "c3_logits"):
        spec = H.iwae_param_spec(hidden=HIDDEN)
        p = H.make_params(spec, 1)
        opt = torch.optim.Adam([p[n] for n, _ in spec], 1e-3)
        x = torch.tensor((rng.uniform(size=(BATCH_PER_GPU, X_DIM)) < 0.5).astype(np.float32))

        def step():
            torch.randn(PARTICLES, BATCH_PER_GPU, Z_DIM)      # the draw the objective discards
            eps = torch.randn(PARTICLES, BATCH_PER_GPU, Z_DIM)
            loss, _ = O.iwae_loss(p, x, eps, PARTICLES, "vimco")
            opt.zero_grad()
            loss.backward()
            if optimizer:
                opt.step()
        return step, BATCH_PER_GPU * PARTICLES
    if name == "c2":
        spec = H.vae_param_spec()
        p = H.make_params(spec, 1)
        opt = torch.optim.Adam([p[n] for n, _ in spec], 1e-3)
        x = torch.tensor((rng.uniform(size=(512, X_DIM)) < 0.5).astype(np.float32))

        def step():
            torch.randn(512, Z_DIM)
            loss, _ = O.vae_loss(p, x, torch.randn(512, Z_DIM))
            opt.zero_grad()
            loss.backward()
            if optimizer:
                opt.step()
        return step, 512
    if name == "c5":
        wm, wl, yl = H.bnn_params(512, 10)
        opt = torch.optim.Adam(wm + wl + [yl], 1e-3)
        xb, yb = torch.randn(512, 13), torch.randn(512)

        def step():
            torch.randn(10, 50, 14)
            torch.randn(10, 1, 51)
            eps = [torch.randn(10, 50, 14), torch.randn(10, 1, 51)]
            loss, _ = O.bnn_loss(wm, wl, yl, xb, yb, eps, 10)
            opt.zero_grad()
            loss.backward()
            if optimizer:
                opt.step()
        return step, 5120
    raise ValueError(name)


def cpu_baseline(name="c3", budget_s=8.0, one_thread_budget_s=5.0, max_steps=40, fwd_bwd_budget_s=4.0):
    """The CPU oracle (torch-CPU restatement of the reference's op sequence, pinned to the reference by
    tests/test_oracle_golden.py) on workload `name`: forward + backward + Adam on this host's cores, at the fastest
    intra-op thread count (calibrated: all cores is often NOT the fastest -- on a 256-thread box the unfused elementwise
    passes run 50x slower with 256 torch threads than with 16-32) and with ONE thread."""
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    step, evals = cpu_step_fn(name)

    def timed(budget, step=step):
        step()
        n, t0 = 0, time.perf_counter()
        while n < max_steps and (n < 2 or (time.perf_counter() - t0) < budget):
            step()
            n += 1
        return n, time.perf_counter() - t0
    best = None
    for nt in sorted({c for c in (4, 8, 16, 32, 64) if c <= avail} or {avail}):
        torch.set_num_threads(nt)
        step()
        t0 = time.perf_counter()
        step()
        dt = time.perf_counter() - t0
        if best is None or dt < best[1]:
            best = (nt, dt)
        if dt > 3.0:
            break
    torch.set_num_threads(best[0])
    n, dt = timed(budget_s)
    rec = {"value": evals * n / dt, "unit": "ELBO-evals/s", "cores": torch.get_num_threads(), "kind": "port",
           "ms_per_step": 1e3 * dt / n, "host_cpus_available": avail, "cpu_model": cpu_model_name(),
           "sample": "%d full training steps (fwd+bwd+Adam) of the same workload, torch-CPU fp32 oracle, %.1f s" % (n, dt),
           "includes": "objective forward + backward + torch.optim.Adam update, like the GPU step it stands beside (the CPU table "
                       "of SURVEY.md section 6 / BASELINE.md times forward + backward only: no optimizer)"}
    if fwd_bwd_budget_s:
        # forward + backward ONLY (no optimizer), same thread count: the quantity BASELINE.md's CPU table holds for the reference
        # itself (35.2 k evals/s at C3 on the build container's 8 cores: iwae.py:157-160-style steps without the update)
        fb_step, _ = cpu_step_fn(name, optimizer=False)
        nf, dtf = timed(fwd_bwd_budget_s, fb_step)
        rec["fwd_bwd_only"] = {"value": evals * nf / dtf, "unit": "ELBO-evals/s", "cores": torch.get_num_threads(),
                               "ms_per_step": 1e3 * dtf / nf, "sample": "%d steps of forward + backward without the optimizer, %.1f s" % (nf, dtf)}
    torch.set_num_threads(1)
    n1, dt1 = timed(one_thread_budget_s)
    rec["one_thread"] = {"value": evals * n1 / dt1, "unit": "ELBO-evals/s", "cores": 1, "ms_per_step": 1e3 * dt1 / n1,
                         "sample": "%d steps, %.1f s" % (n1, dt1)}
    torch.set_num_threads(best[0])
    return rec


# ------------------------------------------------------------------------------------------------ timing helpers
def timed_trials(step, steps, world, dev, min_seconds=0.0, max_trials=200, kick=None):
    """Trials of exactly `steps` steps, each bracketed by synchronize + barrier and reduced with MAX over the ranks;
    at least three (or `max_trials` if fewer) and as many as it takes to cover `min_seconds`.
    Returns (list of elapsed seconds per trial, last loss)."""
    def one():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        last = None
        for _ in range(steps):
            last = step()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, last
    trials = []
    last = None
    # (every rank sees the same, rank-reduced, elapsed times, so every rank stops after the same trial)
    while len(trials) < max_trials and (len(trials) < 3 or sum(trials) < min_seconds):
        if kick is not None:
            kick("timed trial %d" % len(trials))
        el, last = one()
        trials.append(el)
    return trials, last


def make_optimizer(model, torch_adam, groups=None):
    """Adam, lr 1e-3 (the reference callers' optimizer, iwae.py:141): zhusuan.optim.FlatAdam -- the same update over flat
    buckets, one launch per bucket -- or torch.optim.Adam(fused, capturable) with --torch-adam.  `groups`: parameter
    lists that should be one bucket each (the stages of dataparallel.StagedBuckets)."""
    if torch_adam == "reference":          # torch.optim.Adam(model.parameters(), lr): the reference example's line (iwae.py:141)
        return torch.optim.Adam(model.parameters(), 1e-3)
    if torch_adam == "reference_capturable":      # ... with the one flag torch needs to let a step be captured in a graph
        return torch.optim.Adam(model.parameters(), 1e-3, capturable=True)
    if torch_adam:
        return torch.optim.Adam(model.parameters(), 1e-3, fused=True, capturable=True)
    import zhusuan
    return zhusuan.optim.FlatAdam(groups if groups is not None else model.parameters(), lr=1e-3)


def run_single_gpu_config(name, dev, steps, warmup, tuned=True, torch_adam=False, fused_logits=False, skip_discarded=False,
                          dense="fused", eager=False, refresh=False, device_rng=True, forward_only=False, pair_draws=True,
                          steps_per_replay=1):
    """A workload on this GPU as full training steps -- replayed from one hipGraph (default) or launched eagerly from a
    Python loop (`eager`).  `refresh`: every step trains on ANOTHER minibatch, copied (device to device) into the step's
    input tensors from a resident stream of 8 batches, as the reference's loop feeds one (iwae.py:151-160).  `torch_adam`:
    False (zhusuan.optim.FlatAdam), True (torch's fused capturable Adam), "reference" / "reference_capturable"
    (torch.optim.Adam(params, lr) as the reference's example constructs it).  `device_rng`: the draws' Philox state lives in
    device memory (needed by graphs); without it they take their call ids from torch's generator, as plain eager code does.
    `forward_only`: a "step" is ONE EVALUATION OF THE OBJECTIVE (no backward, no optimizer): SURVEY.md 8d's metric (i).
    `pair_draws=False`: zhusuan.pair_draws(False) -- the two draws of a latent as two launches (the package pairs them by default).
    `steps_per_replay` N > 1: zhusuan.GraphedStep(steps_per_replay=N) -- N consecutive training steps recorded into the one graph (the
    ~8.5 us the GPU idles between two graph launches are paid once per N steps); every step is still executed and counted."""
    import contextlib
    import zhusuan
    gemm_tuning(tuned)
    torch.manual_seed(0)
    model, obs, evals, label = make_workload(name, dev, fused_logits=fused_logits, dense=dense)
    opt = None if forward_only else make_optimizer(model, torch_adam)
    rng = zhusuan.DeviceRNG(dev, seed=1) if (device_rng or not eager) else None
    stream = None
    if refresh:
        g = torch.Generator(device="cpu").manual_seed(7)
        stream = dict((k, [v[torch.randperm(v.shape[0], generator=g).to(v.device)].contiguous() for _ in range(8)]) for k, v in obs.items())
    counter = [0]
    one = torch.ones((), device=dev)          # backward's seed, allocated once (loss.backward() fills a fresh one per step)

    def compute():
        if rng is not None:
            rng.begin_step()
        if forward_only:
            with torch.no_grad():
                return model(obs)
        for p in model.parameters():
            p.grad = None
        loss = model(obs)
        loss.backward(one)
        return loss.detach()

    def next_batch():
        i = counter[0] = (counter[0] + 1) % 8
        return dict((k, v[i]) for k, v in stream.items())
    with contextlib.ExitStack() as ctx:
        if rng is not None:
            ctx.enter_context(zhusuan.device_rng(rng))
        ctx.enter_context(zhusuan.skip_discarded_draws(skip_discarded))
        ctx.enter_context(zhusuan.pair_draws(pair_draws))
        if eager:
            def step():
                if refresh:
                    for k, v in next_batch().items():
                        obs[k].copy_(v, non_blocking=True)
                loss = compute()
                if opt is not None:
                    opt.step()
                return loss
            for _ in range(max(3, min(warmup, 10)) + 3):
                step()
        else:
            graphed = zhusuan.GraphedStep(compute, None if opt is None else opt.step, rng=rng, warmup=max(3, min(warmup, 10)), inputs=obs,
                                          steps_per_replay=steps_per_replay)
            step = (lambda: graphed(**next_batch())) if refresh else graphed
        gemm_tuning(tuned, tune=False)       # every GEMM shape of the step has been seen: keep the picks, stop timing
        for _ in range(3):
            step()
        n_calls = max(steps // steps_per_replay, 1)          # (one call = steps_per_replay steps)
        trials, last = timed_trials(step, n_calls, 1, dev, min_seconds=0.3)
        steps = n_calls * steps_per_replay
    med = float(np.median(trials))
    assert np.isfinite(float(last))
    opt_label = {False: "zhusuan.optim.FlatAdam", True: "torch.optim.Adam(fused=True, capturable=True)",
                 "reference": "torch.optim.Adam(params, lr) (the reference example's line)",
                 "reference_capturable": "torch.optim.Adam(params, lr, capturable=True)"}[torch_adam]
    if forward_only:
        opt_label = "none (objective evaluation only: forward under no_grad)"
    return {"workload": label, "ms_per_step": 1e3 * med / steps, "value": evals * steps / med, "unit": "ELBO-evals/s",
            "launch_mode": "eager (Python loop)" if eager else ("hipgraph" if steps_per_replay == 1 else "hipgraph, %d steps per replay" % steps_per_replay), "steps": steps, "trials": len(trials), "final_loss": float(last),
            "minibatch": "a new minibatch every step (8 resident batches, copied into the step's inputs)" if refresh else "one resident minibatch",
            "discarded_draws": "skipped (zhusuan.skip_discarded_draws)" if skip_discarded else (
                "executed (the package default)" if pair_draws else "executed, one launch per draw (zhusuan.pair_draws(False))"),
            "dense_layers": DENSE_LABEL[dense],
            "mlp_gemm_selection": "TunableOp (fastest fp32 solution per shape)" if tuned else "PyTorch default",
            "optimizer": opt_label}


def dp_step_on_one_rank(args, headline_value, timeout_s=240):
    """extra_configs.c3_dp_step_n1: the headline's settings through the DEFAULT MULTI-RANK FORM of the step (flat bucket filled
    by the backward pass, graph A -> all-reduce over RCCL on the compute stream -> graph B = the update) with ONE rank -- the
    fixed cost of the data-parallel path, which caps the 1 -> 8 curve before a byte crosses xGMI and is the only part of that
    curve one GPU can measure.  Runs in a CHILD process (this one never initialises a process group), which also replays the
    same model as a single graph, alternating, for a ratio free of process-to-process differences (`same_process`)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--force-collective-path", "--full", "--no-extras", "--no-cpu-baseline", "--full-record", os.devnull]
    if not args.no_gemm_tuning:
        cmd += ["--gemm-picks", save_gemm_picks(gemm_picks_file("all"))]          # the child runs THIS process's GEMM kernels
    for flag, on in (("--fused-logits", args.fused_logits), ("--torch-adam", args.torch_adam), ("--torch-linear", args.torch_linear),
                     ("--no-gemm-tuning", args.no_gemm_tuning), ("--skip-discarded-draws", args.skip_discarded_draws),
                     ("--allow-experiments", args.allow_experiments), ("--unfused-activations", args.unfused_activations)):
        if on:
            cmd.append(flag)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout_s)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError("the one-rank collective-path run ended with code %d: %s" % (r.returncode, (r.stderr or r.stdout)[-300:]))
    rec = json.loads(lines[-1])
    sp = rec.get("same_process") or {}
    return {"workload": rec["config"]["workload"], "ms_per_step": rec["ms_per_step"], "value": rec["value"], "unit": rec["unit"],
            "vs_headline": rec["value"] / headline_value, "launch_mode": rec["config"]["launch_mode"],
            "collective_library": rec.get("collective_library"), "collective_path": rec.get("collective_path"),
            "parallelism": rec["config"]["parallelism"], "final_loss": rec.get("final_loss"),
            "mlp_gemm_selection": rec["config"].get("mlp_gemm_selection"),
            "same_process_single_graph_ms": sp.get("single_graph_ms_per_step"),
            "same_process_collective_path_ms": sp.get("collective_path_ms_per_step"),
            "same_process_ratio": sp.get("collective_path_vs_single_graph"), "extra_us_per_step": sp.get("extra_us_per_step")}


DENSE_LABEL = {"fused": "zhusuan.Linear in zhusuan.Sequential (ReLU in the GEMM epilogue; activation backward + bias gradient: AB1)",
               "zhusuan": "zhusuan.Linear in torch.nn.Sequential (bias gradient: CS1; torch's activation passes)",
               "torch": "torch.nn.Linear in torch.nn.Sequential"}


def _timed_launches(klib, out, launches):
    def timed(entry, nbytes, fn, rows, width, key=None, idle_s=0.0):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if idle_s > 0:
            time.sleep(idle_s)           # the shader clock falls back while the GPU idles (the K1 cold figures)
        klib.prof_enable(True)
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()
        klib.prof_enable(False)
        d = sorted(1e3 * v for v in klib.prof_durations(entry))
        med = d[len(d) // 2]
        avg = sum(d) / len(d)
        out[key or entry] = {"rows": rows, "row_length": width, "algorithmic_bytes": nbytes, "median_us": med, "min_us": d[0],
                             "avg_us": avg, "launches": len(d), "GBps": nbytes / med / 1e3,
                             "frac_of_hbm_peak": nbytes / med / 1e3 / HBM_PEAK_GBS, "frac_of_hbm_peak_avg": nbytes / avg / 1e3 / HBM_PEAK_GBS}
    return timed


def k1_resident(klib, dev, launches=30):
    """K1 -- the fused Normal sample + log-prob kernel BASELINE.json's north_star sets its >= 60 % target on -- with in-kernel
    Philox at 1 M and 4.2 M rows of D = 40 (179 / 715 MB written), median of `launches` back-to-back launches, HIP events bound
    to each dispatch.  The kernel is bound by VALU issue, i.e. by the shader clock, and the clock follows the recent load: the
    same 4.2 M-row launch takes 183-187 us right after a second of idling (process start, or the CPU-side pauses of a bench run)
    and 125-135 us after 0.3 s of continuous launches (tools/k1_clock_probe.py).  So each size is measured at the SUSTAINED
    clock: back-to-back launches of the same kernel immediately before the timed ones, until their rate has stopped improving."""
    import ctypes
    from zhusuan import _hip
    P = _hip.ptr
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    timed = _timed_launches(klib, out, launches)
    K, D = PARTICLES, Z_DIM
    for B, key in ((20971, "zs_normal_sample_logprob_f32@1M"), (83886, "zs_normal_sample_logprob_f32")):
        N, M = K * B, B * D
        mu, sg = torch.randn(M, device=dev), torch.rand(M, device=dev) + 0.5
        z, lp = torch.empty(K * M, device=dev), torch.empty(B * K, device=dev)
        fn = lambda: klib.call("zs_normal_sample_logprob_f32", P(mu), P(sg), None, 1, 2, None, P(z), P(lp), K, M, D, 1, K, 0, None, st)
        # COLD: the same 30 launches right after a second of idling -- the condition of a kernel sweep, or of a training loop
        # that waits for its data; the clock ramps up inside these launches (roofline.k1_frac_*_cold = bytes / their AVERAGE)
        timed("zs_normal_sample_logprob_f32", 4 * N * D + 4 * N + 8 * M, fn, N, D, key=key + ("" if "@" in key else "@4M") + "_cold", idle_s=1.0)
        # sustained clock (see the docstring): 50 ms windows of back-to-back launches until six windows in a row bring no
        # improvement of more than 1 % (at least 1 s, at most 4 s: on some boxes the ramp from a cold process is slow -- one box
        # showed 58.5 % at 1 M rows after 0.3 s where the sweep in the same call, seconds of launches later, measured 63.3 %)
        t0, best, flat = time.perf_counter(), float("inf"), 0
        while True:
            w0, n = time.perf_counter(), 0
            while time.perf_counter() - w0 < 0.05:
                for _ in range(20):
                    fn()
                torch.cuda.synchronize()
                n += 20
            per = (time.perf_counter() - w0) / n
            best, flat = (per, 0) if per < 0.99 * best else (best, flat + 1)
            el = time.perf_counter() - t0
            if (el >= 1.0 and flat >= 6) or el >= 4.0:
                break
        timed("zs_normal_sample_logprob_f32", 4 * N * D + 4 * N + 8 * M, fn, N, D, key=key)
        del mu, sg, z, lp
    torch.cuda.empty_cache()
    return out


def hbm_resident_kernels(klib, dev, launches=30):
    """The streaming kernels on working sets that cannot sit in the 256 MiB Infinity Cache (the config-size figures in
    `hip_kernels` can: 41 / 81 MB), in this same process: K3 forward / backward at N = 131 050 rows x 784 (420 / 831 MB).
    Median of `launches` (30) back-to-back launches, HIP events bound to each dispatch.  (K1: k1_resident, measured first.)"""
    import ctypes
    from zhusuan import _hip
    P = _hip.ptr
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    timed = _timed_launches(klib, out, launches)
    K = PARTICLES
    B, X = 2621, X_DIM
    N = K * B
    p = torch.rand(N * X, device=dev) * 0.96 + 0.02
    x = (torch.rand(B * X, device=dev) < 0.5).float()
    lp = torch.empty(B * K, device=dev)
    glp = torch.randn(B * K, device=dev)
    gp = torch.empty(N * X, device=dev)
    timed("zs_bernoulli_logprob_f32", 4 * N * X + 4 * B * X + 4 * N,
          lambda: klib.call("zs_bernoulli_logprob_f32", P(p), P(x), B * X, P(lp), K, B, X, 1, K, st), N, X)
    timed("zs_bernoulli_logprob_bwd_f32", 8 * N * X + 4 * B * X + 4 * N,
          lambda: klib.call("zs_bernoulli_logprob_bwd_f32", P(p), P(x), B * X, P(glp), 1, K, P(gp), K, B, X, st), N, X)
    p.mul_(8.0).sub_(4.0)                      # the same buffer as logits
    timed("zs_bernoulli_logits_logprob_f32", 4 * N * X + 4 * B * X + 4 * N,
          lambda: klib.call("zs_bernoulli_logits_logprob_f32", P(p), P(x), B * X, P(lp), None, K, B, X, 1, K, st), N, X)
    timed("zs_bernoulli_logits_logprob_bwd_f32", 8 * N * X + 4 * B * X + 4 * N,
          lambda: klib.call("zs_bernoulli_logits_logprob_bwd_f32", P(p), P(x), B * X, P(glp), 1, K, P(gp), K, B, X, st), N, X)
    del p, gp, x
    del lp, glp
    # K3 forward alone at the CONFIG size (12 800 rows, 41 MB: inside the Infinity Cache), the mapping VERDICT r03 weak 3 is about
    Bc = BATCH_PER_GPU
    Nc = K * Bc
    pc = torch.rand(Nc * X, device=dev) * 0.96 + 0.02
    xc = (torch.rand(Bc * X, device=dev) < 0.5).float()
    lpc = torch.empty(Bc * K, device=dev)
    timed("zs_bernoulli_logprob_f32", 4 * Nc * X + 4 * Bc * X + 4 * Nc,
          lambda: klib.call("zs_bernoulli_logprob_f32", P(pc), P(xc), Bc * X, P(lpc), K, Bc, X, 1, K, st), Nc, X,
          key="zs_bernoulli_logprob_f32@config")
    del pc, xc, lpc
    torch.cuda.empty_cache()
    return out


# kernel-name fragment -> C-ABI entry point (most specific first); logits forms carry <true, ...> as first template argument
# (the kernels shared by the location-scale families live in namespace zs: first template argument 0 = Normal, 1 = Logistic)
_KERNEL_ENTRY = [("k_iw1_persist", "zs_bernoulli_iw_objective_f32"), ("k_iw1_block", "zs_bernoulli_iw_objective_f32"),
                 ("k_iw1_bwd", "zs_bernoulli_iw_objective_bwd_f32"),
                 ("k_column_sum", "zs_column_sum_f32"), ("k_logjoint_bwd", "zs_logjoint_scalar_bwd_f32"), ("k_logjoint_fwd", "zs_logjoint_scalar_f32"),
                 ("k_normal_sample_multi_bwd", "zs_normal_sample_logprob_multi_bwd_f32"),
                 ("k_normal_sample_multi", "zs_normal_sample_logprob_multi_f32"),
                 ("k_particle_linear_bwd", "zs_particle_linear_bwd_f32"), ("k_particle_linear", "zs_particle_linear_f32"),
                 ("k_particle_mlp_bwd", "zs_particle_mlp_bwd_f32"), ("k_particle_mlp", "zs_particle_mlp_f32"), ("k_particle_rmse", "zs_particle_rmse_f32"),
                 ("k_bern_logprob_bwd", "zs_bernoulli%s_logprob_bwd_f32"), ("k_bern_logprob", "zs_bernoulli%s_logprob_f32"),
                 ("k_sample_tile<0", "zs_normal_sample_logprob_f32"), ("k_sample_tile<1", "zs_logistic_sample_logprob_f32"),
                 ("k_logprob_bwd_ksum<0", "zs_normal_logprob_bwd_ksum_f32"), ("k_logprob_krep<0", "zs_normal_logprob_f32"),
                 ("k_adam_step", "zs_adam_step_f32"),
                 ("k_normal_sample_bwd", "zs_normal_sample_logprob_bwd_f32"), ("k_normal_sample", "zs_normal_sample_logprob_f32"),
                 ("k_normal_logprob_bwd_ksum", "zs_normal_logprob_bwd_ksum_f32"), ("k_normal_logprob_bwd", "zs_normal_logprob_bwd_f32"),
                 ("k_normal_logprob", "zs_normal_logprob_f32"), ("k_iw_reduce", "zs_iw_reduce_f32"), ("k_lme", "zs_log_mean_exp_f32")]


def _entry_of_kernel(name):
    for frag, entry in _KERNEL_ENTRY:
        i = name.find(frag)
        if i >= 0:
            if frag == "k_column_sum":          # k_column_sum<T, V, ACT>: ACT != 0 is AB1 (activation backward + column sum)
                targs = name[name.find("<", i) + 1:name.find(">", i)].replace(" ", "").split(",")
                return entry if len(targs) < 3 or targs[2] == "0" else "zs_dense_act_bwd_f32"
            if "%s" in entry:
                j = name.find("<", i)
                logits = j >= 0 and name[j + 1:j + 5] == "true"
                return entry % ("_logits" if logits else "")
            return entry
    return None


def device_kernel_times(run_steps, n_steps):
    """Per-entry-point kernel durations of `n_steps` steps in the launch mode of the timed region (hipGraph replays
    included), from the device timestamps of every dispatch collected in-process by torch.profiler (roctracer).
    HIP events cannot do this: neither hipExtLaunchKernelGGL's start/stop events nor event-record nodes survive stream
    capture (tools/graph_event_probe.hip).  Returns {} when the tracer is unavailable (e.g. rocprofv3 attached)."""
    done = [False]
    try:
        from torch.profiler import profile, ProfilerActivity
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                run_steps(n_steps)
                done[0] = True
                torch.cuda.synchronize()
            acc = {}
            for e in prof.events():
                entry = _entry_of_kernel(e.name)
                if entry is None:
                    continue
                d = getattr(e, "device_time", None)
                if d is None:
                    d = getattr(e, "cuda_time", 0.0)
                if d and d > 0:
                    acc.setdefault(entry, []).append(float(d))
        return dict((k, {"avg_us": sum(v) / len(v), "min_us": min(v), "count": len(v)}) for k, v in acc.items())
    except Exception as e:                                          # noqa: BLE001
        sys.stderr.write("bench: in-process device tracing unavailable (%r); using HIP-event timing of eager launches\n" % (e,))
        if not done[0]:
            # with several ranks the steps hold collectives: this rank must run as many as its peers, tracer or not.  (A tracer
            # that fails to START has run none; run_steps itself raising is a real error and propagates from here.)
            run_steps(n_steps)
            torch.cuda.synchronize()
        return {}


COLLECTIVE_TIMEOUT_S = 180      # process-group timeout: rendezvous, and every collective under RCCL's watchdog


class Watchdog(object):
    """A multi-rank run must END, with a reason, whatever goes wrong on a node nobody can log in to.  Every stage of main()
    calls kick(name); a daemon thread checks the time since the last kick and, past the limit, writes ONE line to stderr
    (rank, stage, seconds) and leaves with os._exit(5) -- torch.distributed.run then tears the other ranks down.  Nothing is
    re-exec'ed, nothing is retried.  (The process group's own timeout catches a collective that never completes under RCCL;
    this catches everything else: a rank waiting in a barrier for a peer that died silently, a stuck capture, a wedged
    host thread.)"""

    def __init__(self, rank, limit_s):
        import threading
        self.rank, self.limit, self.stage, self.t = rank, float(limit_s), "start", time.monotonic()
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, name="bench-watchdog", daemon=True)
        self._thread.start()

    def kick(self, stage):
        self.stage, self.t = stage, time.monotonic()

    def stop(self):
        self._stop.set()

    def _run(self):
        while not self._stop.wait(1.0):
            waited = time.monotonic() - self.t
            if waited > self.limit:
                sys.stderr.write("bench: rank %d made no progress for %.0f s in stage '%s' (limit %.0f s): giving up, exit code 5\n"
                                 % (self.rank, waited, self.stage, self.limit))
                sys.stderr.flush()
                os._exit(5)


def fail(rank, what, exc=None):
    """One line, non-zero exit (the launcher ends the other ranks); never re-exec, never continue half-configured."""
    sys.stderr.write("bench: rank %d: %s%s\n" % (rank, what, (": %r" % (exc,)) if exc is not None else ""))
    sys.stderr.flush()
    raise SystemExit(3)


def short(e, limit=150):
    """An exception for the one-line record: type and the head of its message (the full text goes to stderr)."""
    t = repr(e)
    sys.stderr.write("bench: %s\n" % t[:4000])
    return t if len(t) <= limit else t[:limit - 3] + "..."


LINE_LIMIT = 8192


def fit_line(out, limit=LINE_LIMIT):
    """The one-line record, ALWAYS printed and always under `limit` bytes (the driver keeps a tail of stdout).  Error texts were
    cut when they were recorded (`short`); if the line is still too long -- many failing extras -- the optional parts go, least
    important first, and the line says which (`dropped_from_line`; the full record keeps everything).  Never an assertion:
    the run that needs its diagnostics most is the one with failures in it."""
    line = json.dumps(out)
    if len(line) <= limit:
        return line
    out = dict(out)
    dropped = []
    ex = dict(out.get("extra_configs") or {})
    order = sorted(ex, key=lambda k: ("error" not in ex[k], k))      # failed extras first (their text is in the full record)
    while order and len(json.dumps(dict(out, extra_configs=ex, dropped_from_line=dropped))) > limit:
        key = order.pop(0)
        ex.pop(key)
        dropped.append("extra_configs." + key)
    out["extra_configs"] = ex
    for key in ("env_overrides", "library", "cpu_baseline"):
        out["dropped_from_line"] = dropped
        if len(json.dumps(out)) <= limit:
            break
        if key in out:
            out[key] = None if key == "cpu_baseline" else "see full_record"
            dropped.append(key)
    out["dropped_from_line"] = dropped
    line = json.dumps(out)
    if len(line) > limit:                      # the contract keys alone (cannot be reached with sane values)
        keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "full_record")
        line = json.dumps(dict(((k, out.get(k)) for k in keep), config={"workload": str(out.get("config", {}).get("workload"))[:200]},
                               roofline=None, cpu_baseline=None, dropped_from_line=["everything else"]))
    return line


def dump_outputs(directory, model, loss, grad_scale):
    """--dump-outputs: what the last timed step computed, as its caller receives it -- `loss` (the objective, float64, 0-d),
    `iw_bound` (the forward's per-datapoint importance-weighted bound), `param.<name>` (every parameter after the step's update) and
    `grad.<name>` (the gradients of the step's backward, averaged over the ranks) -- one float32 / float64 .npy each, about 11 MB
    at the headline shape.  The inputs (data, initial weights, Philox streams) are seeded and the GEMM kernels are the committed
    picks (gemm_tuning): the same arguments give the same arrays, bit for bit."""
    os.makedirs(directory, exist_ok=True)
    arrays = {"loss": np.asarray(loss, dtype=np.float64), "iw_bound": model.last_iw_bound.detach().float().cpu().numpy()}
    for name, p in model.named_parameters():
        arrays["param." + name] = p.detach().float().cpu().numpy()
        if p.grad is not None:
            arrays["grad." + name] = (p.grad.detach().float() * grad_scale).cpu().numpy()
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), a)


def main():
    args = parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench: --gpus %d but the launcher started %d ranks" % (args.gpus, world))
    global BATCH_PER_GPU
    if args.batch_per_gpu > 0:
        BATCH_PER_GPU = args.batch_per_gpu
    if args.strong_scaling:
        if 2048 % world:
            raise SystemExit("bench: --strong-scaling splits 2048 datapoints; %d ranks do not divide it" % world)
        BATCH_PER_GPU = 2048 // world
    # test hook (tests/test_bench_contract.py): several ranks share GPU 0 and talk over gloo, so that the multi-rank
    # control flow (shards, buckets, staged graphs, max-over-ranks timing) can be exercised on a one-GPU box.  RCCL
    # refuses two ranks on one device, so this is never a measurement mode.
    share_device = os.environ.get("ZS_BENCH_SHARE_DEVICE") == "1"
    dev_index = 0 if share_device else local_rank
    if not share_device and torch.cuda.device_count() <= dev_index:
        raise SystemExit("bench: rank %d needs GPU %d, this node exposes %d" % (rank, dev_index, torch.cuda.device_count()))
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    wd = Watchdog(rank, float(os.environ.get("ZS_BENCH_WATCHDOG_S", "600"))) if world > 1 else None
    kick = wd.kick if wd is not None else (lambda stage: None)
    if world > 1 or (args.force_collective_path and "RANK" in os.environ):
        import datetime
        kick("init_process_group")
        try:
            if share_device:
                dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=COLLECTIVE_TIMEOUT_S))
            else:
                dist.init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(seconds=COLLECTIVE_TIMEOUT_S))
            # the first collective builds the communicator (RCCL: rings over xGMI, dmabuf IPC handles): do it HERE, where a
            # failure has one obvious meaning, not inside the first training step
            kick("first collective (communicator set-up)")
            probe = torch.ones(1, device=dev)
            dist.all_reduce(probe)
            torch.cuda.synchronize()
            if int(probe.item()) != world:
                fail(rank, "the first all-reduce over %d ranks returned %r" % (world, probe.item()))
        except SystemExit:
            raise
        except Exception as e:                                      # noqa: BLE001
            fail(rank, "process group set-up failed (backend %s, %d ranks, HSA_ENABLE_IPC_MODE_LEGACY=%s)"
                 % ("gloo" if share_device else "nccl", world, os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")), e)

    if args.blas != "default":
        torch.backends.cuda.preferred_blas_library("cublaslt" if args.blas == "hipblaslt" else "cublas")
    tuned = gemm_tuning(not args.no_gemm_tuning, picks=args.gemm_picks or None)
    import zhusuan  # noqa: F401
    from zhusuan import _hip, dataparallel
    if args.iw1_max_stream_bytes >= 0:
        from zhusuan import _ops
        _ops.IW1_MAX_STREAM_BYTES = args.iw1_max_stream_bytes

    k1_first = {}
    if args.full and world == 1 and rank == 0 and not args.no_extras and not args.force_collective_path:
        try:
            k1_first = k1_resident(_hip.lib(), dev)
        except Exception as e:                                      # noqa: BLE001
            k1_first = {"error": short(e)}
    torch.manual_seed(0)
    dense = "torch" if args.torch_linear else ("zhusuan" if args.unfused_activations else "fused")
    model, obs, evals_per_step, _ = make_workload("c3", dev, seed_rank=rank, fused_logits=args.fused_logits, dense=dense)
    dataparallel.broadcast_parameters(model)
    rng = zhusuan.DeviceRNG(dev, seed=1000 + rank)          # per-rank Philox stream, state in device memory

    multi = world > 1 or args.force_collective_path
    hooks = multi and args.no_graph and args.overlap_allreduce
    staged = multi and not args.no_graph and args.overlap
    # The data path's collective: this job's own RCCL communicator, driven on the compute stream with no event around it
    # (collective set-up: every rank, here; a communicator on every rank or on none -- then torch.distributed's all_reduce)
    rccl = None
    if multi and dist.is_initialized() and not share_device and not args.no_direct_rccl:
        kick("RCCL communicator of the data path")
        rccl = dataparallel.DirectAllReduce.create(timeout_s=120.0)
        if rccl is None and rank == 0:
            sys.stderr.write("bench: direct RCCL communicator unavailable (%s); all-reducing through torch.distributed\n"
                             % dataparallel.DirectAllReduce.last_error)
    # Gradients are written into the flat buckets by the backward pass itself (direct=True: the dense layers' weight GEMMs and
    # bias reductions take the bucket slices as their outputs), so no concatenation pass runs before a collective; with one
    # rank and no collective there is no bucket to fill.  (One registration per parameter: only the form in use registers.)
    bucket = dataparallel.GradientBucket(model, direct=multi and not staged and not hooks)
    obuckets = dataparallel.OverlappedBuckets(model, n_buckets=2) if hooks else None
    # --overlap: backward reaches the decoder's (generator's) parameters first, then the encoder's: two stages, two buckets;
    # --force-collective-path with one rank issues the all-reduces all the same (what the path costs before a byte moves)
    sbuckets = dataparallel.StagedBuckets([model.generator.parameters(), model.variational.parameters()], direct=True,
                                          always_collective=args.force_collective_path) if staged else None
    # the update reads the summed gradients where the collective left them, 1/world folded into the read (FlatAdam takes a
    # pointer per tensor: one launch whatever the buckets; round 5 launched once per bucket)
    opt = make_optimizer(model, args.torch_adam)
    grad_scale = 1.0 / world
    held = {}

    one = torch.ones((), device=dev)          # backward's seed, allocated once (loss.backward() fills a fresh one per step)

    # Several ranks, tuned GEMMs: ONE tuning run for the job.  Left to themselves the ranks time the fp32 GEMM solutions independently
    # and near-ties come out differently, so replicas run slightly different kernels and the step takes the time of the slowest
    # rank's picks (the same effect put +- 1.5 % between the headline process and its one-rank child).  Rank 0 evaluates the
    # objective's forward + backward three times -- every GEMM shape of the step, no collective involved --, writing its picks where
    # the other ranks (one node: one /tmp) read them after a barrier; a rank that cannot read them tunes for itself as before.
    gemm_picks_shared = None
    if world > 1 and tuned and dist.is_initialized() and os.environ.get("ZS_BENCH_NO_SHARED_PICKS") != "1":
        import tempfile
        shared = os.path.join(tempfile.gettempdir(), "zs_bench_tunableop_job_%s.csv" % os.environ.get("MASTER_PORT", "0"))
        kick("GEMM picks of rank 0")
        try:
            if rank == 0:
                if os.path.exists(shared):
                    os.remove(shared)
                # (torch.autograd.grad, not backward(): the parameters' AccumulateGrad nodes remember the stream they first ran on, and a
                #  first use on the default stream breaks the capture that follows -- a segfault in capture_end, seen once here)
                #  and on a side stream, like the warm-up of the capture itself: nothing of the step touches the default stream before it
                params_ = [p_ for p_ in model.parameters() if p_.requires_grad]
                pre = torch.cuda.Stream()
                pre.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(pre), zhusuan.device_rng(rng):
                    for _ in range(3):
                        rng.begin_step()
                        torch.autograd.grad(model(obs), params_, grad_outputs=one, allow_unused=True)
                torch.cuda.current_stream().wait_stream(pre)
                torch.cuda.synchronize()
                save_gemm_picks(shared)
        except Exception as e:                                      # noqa: BLE001
            sys.stderr.write("bench: rank %d: pre-tuning failed (%r); every rank tunes for itself\n" % (rank, e))
        dist.barrier()
        if rank != 0:
            gemm_tuning(True, picks=shared)
        gemm_picks_shared = dataparallel.all_ranks_agree(bool(rank == 0 or GEMM_PICKS["loaded_from"]), device=dev)

    def compute_part():
        """objective forward + backward (+ packing the flat [grads | loss] bucket when there is a collective)"""
        rng.begin_step()
        bucket.zero()
        loss = model(obs)
        loss.backward(one)
        if multi:
            bucket.pack(loss)
        return loss.detach()

    def exchange_part(loss):
        """ONE collective after the whole backward, on the compute stream: all-reduce (SUM) of the flat bucket over RCCL / xGMI.
        Returns the objective's slot: the SUM over the ranks (the line divides by the world size once, after the timed region)."""
        if not multi:
            return loss
        bucket.exchange(direct=rccl, always=args.force_collective_path)
        return bucket.flat[bucket.n_grad]

    def update_part():
        """Adam; the 1/world of the gradient mean rides in FlatAdam's gradient read (torch's Adam: one pass over the bucket first)"""
        if not multi or hooks:
            opt.step()
        elif args.torch_adam:
            bucket.scale()
            opt.step()
        else:
            opt.step(grad_scale=grad_scale)

    def step_body():
        """the step launched eagerly (also what the HIP-event kernel timing pass runs)"""
        if hooks:                         # buckets leave from autograd hooks during backward
            rng.begin_step()
            obuckets.zero()
            loss = model(obs)
            obuckets.begin(loss)
            loss.backward(one)
            g = obuckets.finish()
        else:
            g = exchange_part(compute_part())
        update_part()
        return g

    # the staged step (default with more than one rank): decoder backward | all-reduce bucket 0 (asynchronous, on
    # RCCL's stream) | encoder backward, overlapping it | all-reduce bucket 1, wait | 1/world + Adam
    # (With VIMCO the encoder's gradients do not pass through the decoder: stage 2 repeats nothing but the objective's own
    #  backward.  StagedBuckets.backward_stage(also=..., roots=...) cuts the stages at the variational net's outputs instead --
    #  what a reparameterised objective wants; here it was measured and lost 8 us to the boundary tensors' gradient copies.)
    def stage_forward_and_decoder_backward():
        rng.begin_step()
        sbuckets.zero()
        held["loss"] = model(obs)
        sbuckets.backward_stage(held["loss"], 0)
        return held["loss"].detach()

    def stage_encoder_backward():
        sbuckets.backward_stage(held["loss"], 1)

    def stage_update():
        if args.torch_adam:
            sbuckets.scale()
            opt.step()
        else:                              # the 1/world rides along in the update's gradient read: no pass over the buckets
            sbuckets.scale(gradients=False)
            opt.step(grad_scale=sbuckets.grad_scale())

    skip_discarded = bool(args.skip_discarded_draws)
    klib = _hip.lib()
    if "experiments" in klib.build_info() and not args.allow_experiments:
        raise SystemExit("bench: %s is an experiments build (%s); pass --allow-experiments" % (klib.path, klib.build_info()))
    mode = "eager"
    capture_note = None
    # test hooks (tests/test_bench_contract.py): ONE rank's graph capture fails / ONE rank stops making progress
    fail_capture_rank = int(os.environ.get("ZS_BENCH_FAIL_CAPTURE_RANK", "-1"))
    stall_rank = int(os.environ.get("ZS_BENCH_STALL_RANK", "-1"))

    def maybe_fail_capture():
        if rank == fail_capture_rank and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("capture failure injected on rank %d (ZS_BENCH_FAIL_CAPTURE_RANK)" % rank)

    def agree(ok):
        return dataparallel.all_ranks_agree(ok, device=dev)

    # bucket 1's result is needed by the very next kernel (the update): its all-reduce goes on the compute stream itself (no
    # cross-stream hops), bucket 0's runs beside the encoder's backward and is joined here
    def second_exchange():
        sbuckets.launch(1, overlap=False, direct=rccl)
        sbuckets.wait()

    def eager_staged_step():
        """the staged step without graphs: the SAME stages, hence the same two all-reduces, launched from Python"""
        stage_forward_and_decoder_backward()
        sbuckets.launch(0)
        stage_encoder_backward()
        second_exchange()
        stage_update()
        return sbuckets.loss_slot()

    # what a step returns is the objective's slot of the bucket as the update left it: the SUM over the ranks when the 1/world
    # rode in FlatAdam's gradient read (the line divides once, after the timed region -- no kernel per step for a diagnostic)
    slot_is_sum = multi and not hooks and not args.torch_adam

    with zhusuan.device_rng(rng), zhusuan.skip_discarded_draws(skip_discarded):
        step = step_body
        if args.no_graph:
            for i in range(args.warmup):
                kick("eager warm-up step %d" % i)
                step_body()
        else:
            # The launch-bound inner loop (~130 kernels, most of them a few microseconds) is replayed from hipGraphs
            # (warm-up on the capture stream, thread-local capture mode): ONE graph with a single rank; with a
            # collective, graphs around the eagerly launched RCCL calls.
            #
            # Several ranks decide TOGETHER whether they replay graphs: a rank that fell back to eager launches alone would
            # still have to issue exactly its peers' collectives.  Both fallbacks do (the staged step's fallback runs the same
            # stages eagerly: two all-reduces of the same two buckets; the one-bucket step's fallback is step_body: the same one
            # all-reduce), and the decision itself is an all-reduce (MIN) every rank makes at the same points: after each
            # capture attempt inside GraphedStages / once after GraphedStep's recording.  An exception anywhere ELSE (warm-up,
            # out of memory) ends this rank with a one-line reason and a non-zero exit code; the launcher ends the others.
            kick("graph warm-up and capture")
            captured = True
            try:
                if staged:
                    def first_stage():
                        maybe_fail_capture()
                        return stage_forward_and_decoder_backward()
                    stages = [("graph", first_stage), ("eager", lambda: sbuckets.launch(0)),
                              ("graph", stage_encoder_backward), ("eager", second_exchange),
                              ("graph", stage_update)]
                    gs = zhusuan.GraphedStages(stages, rng=rng, warmup=max(args.warmup, 3), agree=agree if world > 1 else None)
                    captured, capture_note = gs.captured, gs.capture_error

                    def step():
                        gs()
                        return sbuckets.loss_slot()
                    mode = "hipgraph x3, all-reduce of the decoder's gradients overlapped with the encoder's backward"
                else:
                    def compute_graphed():
                        maybe_fail_capture()
                        return compute_part()
                    step = gstep = zhusuan.GraphedStep(compute_graphed, update_part, exchange=exchange_part if multi else None, rng=rng,
                                                       warmup=max(args.warmup, 3), agree=agree if world > 1 else None, optimizer=opt)
                    captured, capture_note = gstep.captured, gstep.capture_error
                    mode = "hipgraph x2 around ONE all-reduce on the compute stream" if multi else "hipgraph"
            except Exception as e:                      # noqa: BLE001
                if world > 1:        # not at a meeting point: the peers may be inside a collective this rank will never join
                    fail(rank, "graph warm-up failed outside a capture (stage '%s')" % (wd.stage if wd else "?"), e)
                captured, capture_note = False, short(e)
                torch.cuda.synchronize()
            if not captured:
                sys.stderr.write("bench: rank %d: graph capture gave way to eager launches on every rank (%s)\n"
                                 % (rank, capture_note or "another rank's capture failed"))
                step = eager_staged_step if staged else step_body
                mode = ("eager (graph capture failed on a rank; all ranks fell back together), %s"
                        % ("two staged all-reduces" if staged else "one all-reduce")) if multi else "eager"
            for i in range(3):
                kick("post-capture step %d" % i)
                step()
        if hooks:
            mode = "eager, all-reduce overlapped with backward from autograd hooks (2 buckets)"
        gemm_tuning(tuned, tune=False)       # the warm-up has seen every GEMM shape of the step: keep the picks, stop timing
        if rank == stall_rank:              # test hook: this rank stops here; its peers wait in the first trial's barrier
            time.sleep(10 ** 6)
        trials, last = timed_trials(step, args.steps, world, dev, max_trials=1, kick=kick)      # exactly --steps timed steps
        # (read here: the same-process twin below trains the same model on -- tools/gpu_job.sh dp_soak compares the forms at equal step counts)
        final_loss = float(last) * (grad_scale if slot_is_sum else 1.0)
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, model, final_loss, grad_scale if slot_is_sum else 1.0)
        # one rank on the collective path: the SAME model, optimizer, GEMM picks and box as a single graph, alternating with
        # the multi-rank form -- what the path costs before a byte crosses xGMI, free of process-to-process differences
        same_process = None
        if args.full and args.force_collective_path and world == 1 and mode.startswith("hipgraph"):
            from zhusuan import _ops

            def compute_single():          # the headline step exactly: gradients allocated by autograd, no bucket involved
                rng.begin_step()
                bucket.zero()
                if sbuckets is not None:
                    sbuckets.zero()
                loss = model(obs)
                with _ops.grad_destinations_paused():
                    loss.backward(one)
                return loss.detach()
            twin = zhusuan.GraphedStep(compute_single, opt.step, rng=rng, warmup=3)
            t_multi, t_single = [], []
            for _ in range(3):
                t_single += timed_trials(twin, args.steps, 1, dev, min_seconds=0.25)[0]
                t_multi += timed_trials(step, args.steps, 1, dev, min_seconds=0.25)[0]
            m_multi, m_single = float(np.median(t_multi)), float(np.median(t_single))
            same_process = {"single_graph_ms_per_step": 1e3 * m_single / args.steps, "collective_path_ms_per_step": 1e3 * m_multi / args.steps,
                            "collective_path_vs_single_graph": m_single / m_multi,
                            "extra_us_per_step": 1e6 * (m_multi - m_single) / args.steps, "trials_each": len(t_multi)}
            del twin
        elapsed = float(np.median(trials))

        def run_steps(n):
            for _ in range(n):
                step()

        if args.full:
            kick("per-kernel timing passes")
            # per-kernel durations: the same steps launched eagerly with start/stop HIP events bound to each
            # kernel dispatch on its stream (events cannot ride inside a graph replay)
            n_prof = min(args.steps, 50)
            # bytes of the callers' layer kernels (AB1 / CS1: one launch per dense layer, shapes differ): their arguments, from the calls
            layer_bytes, real_call = {}, klib.call

            def spy(name, *a):
                if name == "zs_dense_act_bwd_f32":
                    layer_bytes[name] = layer_bytes.get(name, 0) + 12 * a[5] * a[6] + 4 * a[6]       # read g, y; write gpre, bias gradient
                elif name == "zs_column_sum_f32":
                    layer_bytes[name] = layer_bytes.get(name, 0) + 4 * a[2] * a[3] + 4 * a[3]
                return real_call(name, *a)

            def eager_steps(n):
                if mode != "eager" and not hooks:
                    side = torch.cuda.Stream()       # eager launches next to captured graphs: stay off the default stream
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        for _ in range(n):
                            step_body()
                    torch.cuda.current_stream().wait_stream(side)
                else:
                    for _ in range(n):
                        step_body()
                torch.cuda.synchronize()
            klib.call = spy
            try:
                eager_steps(1)
            finally:
                klib.call = real_call
            klib.prof_enable(True)
            eager_steps(n_prof)
            klib.prof_enable(False)
            # the same kernels timed in the launch mode of the timed region (graph replays): device timestamps per dispatch
            n_dev = min(args.steps, 30)
            # an external tracer (rocprofv3) owns the activity records: kineto then returns garbage durations
            external_tracer = any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ) or \
                "rocprofiler-sdk-tool" in os.environ.get("LD_PRELOAD", "")
            if rank == 0 and not external_tracer and os.environ.get("ZS_BENCH_NO_TRACER") != "1":
                dev_times = device_kernel_times(run_steps, n_dev)
            else:
                run_steps(n_dev)
                dev_times = {}
            torch.cuda.synchronize()
        if args.timeline and rank == 0:
            try:
                from torch.profiler import profile, ProfilerActivity
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as tprof:
                    run_steps(5)
                    torch.cuda.synchronize()
                tprof.export_chrome_trace(args.timeline)
            except Exception as e:                                  # noqa: BLE001
                sys.stderr.write("bench: --timeline: %r\n" % (e,))
        elif args.timeline:
            run_steps(5)                 # (the other ranks run the same collectives)
            torch.cuda.synchronize()
        # every replica started from rank 0's weights and applied the same averaged gradients: their parameters must be
        # bit-identical after any number of steps.  A collective that summed the wrong buffers shows up here.
        replicas = None
        if args.full and world > 1 and dist.is_initialized():
            kick("replica check")
            with torch.no_grad():
                flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).double()
                mine = torch.stack([flat.sum(), flat.abs().sum(), (flat * flat).sum()])
            gathered = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(gathered, mine)
            sums = torch.stack(gathered).cpu()
            in_sync = bool((sums == sums[0:1]).all())
            replicas = {"in_sync": in_sync, "ranks": world,
                        "max_checksum_difference": float((sums - sums[0:1]).abs().max())}
            if not in_sync:
                sys.stderr.write("bench: rank %d: REPLICAS DIVERGED: per-rank parameter checksums %r\n" % (rank, sums.tolist()))
    kick("record")
    assert np.isfinite(final_loss)

    if rank == 0:
        N, B, D, X = PARTICLES * BATCH_PER_GPU, BATCH_PER_GPU, Z_DIM, X_DIM
        # algorithmic bytes per launch of each hot-path entry point on this workload
        algo = {
            "zs_bernoulli_logprob_f32": 4 * N * X + 4 * B * X + 4 * N,            # read p once, x once, write N sums
            "zs_bernoulli_logprob_bwd_f32": 8 * N * X + 4 * B * X + 4 * N,        # read p, x, g; write gp
            "zs_bernoulli_logits_logprob_f32": 4 * N * X + 4 * B * X + 4 * N,
            "zs_bernoulli_logits_logprob_bwd_f32": 8 * N * X + 4 * B * X + 4 * N,
            "zs_normal_sample_logprob_f32": 4 * N * D + 4 * N + 8 * B * D,        # write z, log q; read mu, sigma
            "zs_normal_sample_logprob_pair_f32": 2 * (4 * N * D + 4 * N) + 8 * B * D,     # both draws of the latent in one launch
            "zs_normal_logprob_f32": 4 * N * D + 4 * N + 8 * B * D,
            "zs_normal_logprob_bwd_ksum_f32": 4 * N * D + 4 * N + 16 * B * D,
            "zs_iw_reduce_f32": 16 * N + 8 * B,
            "zs_iw_objective_f32": 20 * N + 4 * B + 4,                            # read a, b, q; write [2,B,K] coefficients, bounds, mean
            # IW1: read p, x, z, the prior's parameters, log q; write both row-sum matrices, both coefficient matrices, costs, bounds
            "zs_bernoulli_iw_objective_f32": 4 * N * X + 4 * B * X + 4 * N * D + 8 * B * D + 4 * N + 16 * N + 8 * B + 4,
            # its backward: K3's backward (read p, x, coefficients; write gp) + K2's K-summed backward (read z, mu, sigma, coefficients;
            # write gmu, gsigma) in one launch
            # (beyond 32 768 rows the entry point runs K3's x-reuse backward -- accounted under zs_bernoulli_logprob_bwd_f32, its own
            #  launch -- and only the K-summed log q gradient under this name: --strong-scaling on few ranks)
            "zs_bernoulli_iw_objective_bwd_f32": ((8 * N * X + 4 * B * X + 4 * N) if N <= 32768 else 0) + (4 * N * D + 4 * N + 16 * B * D),
            "zs_adam_step_f32": 28 * sum(p.numel() for p in model.parameters()),  # read p, g, m, v; write p, m, v
        }
        roof = None
        if args.full:
            # the IW kernels serve two entry points; the tracer sees kernel names only
            if "zs_iw_reduce_f32" in dev_times and klib.prof_query("zs_iw_objective_f32")["count"] and \
                    not klib.prof_query("zs_iw_reduce_f32")["count"]:
                dev_times["zs_iw_objective_f32"] = dev_times.pop("zs_iw_reduce_f32")
            # ... and so does the flat-plane sampling kernel (one draw / both draws of a latent)
            if "zs_normal_sample_logprob_f32" in dev_times and klib.prof_query("zs_normal_sample_logprob_pair_f32")["count"] and \
                    not klib.prof_query("zs_normal_sample_logprob_f32")["count"]:
                dev_times["zs_normal_sample_logprob_pair_f32"] = dev_times.pop("zs_normal_sample_logprob_f32")
            per_kernel = {}
            for name in (n for n in _hip.PROTOTYPES if n.endswith("_f32")):     # the workload is fp32 throughout
                q = klib.prof_query(name)
                if q["count"]:
                    avg_ms = q["total_ms"] / q["count"]
                    rec = {"launches_per_step": q["count"] / n_prof, "avg_us": 1e3 * avg_ms, "min_us": 1e3 * q["min_ms"],
                           "us_per_step": 1e3 * q["total_ms"] / n_prof}
                    rec["timing"] = "HIP events, eager launches"
                    dt = dev_times.get(name)
                    if dt and not (0.4 * rec["avg_us"] <= dt["avg_us"] <= 2.5 * rec["avg_us"]):
                        dev_times.pop(name)      # implausible against the HIP-event figure: tracer conflict, ignore
                        dt = None
                    if dt:      # preferred: the kernel as it runs in the timed region's launch mode
                        rec["eager_event_avg_us"] = rec["avg_us"]
                        rec["avg_us"], rec["min_us"] = dt["avg_us"], dt["min_us"]
                        rec["us_per_step"] = dt["avg_us"] * dt["count"] / n_dev
                        rec["timing"] = "device timestamps, %s" % mode
                    if name in layer_bytes and rec["launches_per_step"]:
                        # caller-side layer kernels: several launches of different shapes per step -- bytes and rate of all of them
                        rec["role"] = "caller-side glue (the dense layers' non-GEMM backward passes), not a hot-path row"
                        rec["algorithmic_bytes_per_step"] = layer_bytes[name]
                        rec["GBps"] = layer_bytes[name] / (rec["us_per_step"] * 1e-6) / 1e9
                        rec["frac_of_hbm_peak"] = rec["GBps"] / HBM_PEAK_GBS
                    if name in algo:
                        rec["algorithmic_bytes"] = algo[name]
                        rec["GBps"] = algo[name] / (rec["avg_us"] * 1e-6) / 1e9
                        rec["frac_of_hbm_peak"] = rec["GBps"] / HBM_PEAK_GBS
                        rec["working_set"] = "%.1f MB: inside the 256 MiB Infinity Cache (see hbm_resident for the same kernel " \
                                             "beyond it)" % (algo[name] / 1e6)
                    per_kernel[name] = rec
            # the dominant hot-path kernel of the step = the one that moves the most bytes per step (it is also the
            # one with the most time per step; bytes are used because they do not move when a profiler is attached)
            dominant = max((n for n in per_kernel if n in algo),
                           key=lambda n: algo[n] * per_kernel[n]["launches_per_step"])
            prof = klib.prof_query(dominant)
            ev_ms = prof["total_ms"] / prof["count"]
            if dominant in dev_times:
                k_ms, k_min_ms, k_count = dev_times[dominant]["avg_us"] * 1e-3, dev_times[dominant]["min_us"] * 1e-3, dev_times[dominant]["count"]
                timing = ("device start/end timestamps of each dispatch on its stream, collected in-process (torch.profiler / "
                          "roctracer) over %d steps replayed in the timed region's launch mode (%s) right after it; HIP events "
                          "cannot time a kernel inside a hipGraph replay, their eager-launch figure is eager_event_avg_us" % (n_dev, mode))
            else:
                k_ms, k_min_ms, k_count = ev_ms, prof["min_ms"], prof["count"]
                timing = ("start/stop HIP events bound to each dispatch (hipExtLaunchKernelGGL) on the launch stream, %d steps "
                          "of the same workload launched eagerly right after the timed region" % n_prof)
            algo_bytes = algo[dominant]
            achieved = algo_bytes / (k_ms * 1e-3) / 1e9
            traffic, traffic_source = pmc_traffic(dominant, args.fused_logits, _hip.ABI_VERSION)
            roof = {"bound": "hbm", "kernel": dominant, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": (achieved / HBM_PEAK_GBS) if achieved else None, "traffic": traffic,
                    "algorithmic_bytes_per_launch": algo_bytes, "avg_launch_us": 1e3 * k_ms if k_ms else None,
                    "min_launch_us": 1e3 * k_min_ms, "launches_timed": k_count, "eager_event_avg_us": 1e3 * ev_ms,
                    "timing": "device timestamps per dispatch in the timed region's launch mode (torch.profiler / roctracer)"
                              if dominant in dev_times else "HIP events bound to each dispatch, eager launches"}
        nbytes = sbuckets.nbytes() if staged else (obuckets.nbytes() if hooks else bucket.nbytes())
        settings = {
            "workload": "IWAE-MNIST VIMCO, batch=%d per GPU (global %d), K=%d, latent=%d, x=%d, hidden=%d, full training step "
                        "(fwd+bwd+all-reduce+Adam)" % (BATCH_PER_GPU, BATCH_PER_GPU * world, PARTICLES, Z_DIM, X_DIM, HIDDEN),
            "global_batch": BATCH_PER_GPU * world, "particles": PARTICLES,
            **({"not_a_baseline_config": "--batch-per-gpu %d / --iw1-max-stream-bytes %d: a kernel study, not BASELINE.json's configs[1]"
                % (args.batch_per_gpu, args.iw1_max_stream_bytes)} if (args.batch_per_gpu > 0 or args.iw1_max_stream_bytes >= 0) else {}),
            "parallelism": "dp%d (minibatch shards; %s, %d bytes per step)" % (
                world, "two flat buckets (decoder | encoder gradients + objective)" if (staged or hooks)
                else "one flat bucket [gradients | objective]", nbytes),
            "bernoulli_path": "logits (sigmoid inside the kernel)" if args.fused_logits else "probs (nn.Sigmoid pass, as the reference's example)",
            "dense_layers": DENSE_LABEL[dense],
            "mlp_gemm_library": args.blas,
            "mlp_gemm_selection": ("TunableOp (fastest fp32 solution per shape, callers' nn.Linear stack)" +
                                   (": the picks committed in bench_gemm_picks.csv" if GEMM_PICKS["loaded_from"] == DEFAULT_GEMM_PICKS else
                                    ": the picks of the parent process" if (GEMM_PICKS["loaded_from"] and world == 1) else "") +
                                   ("; one tuning run for the job (rank 0's picks on every rank)" if gemm_picks_shared else "")) if tuned else "PyTorch default",
            "optimizer": "torch.optim.Adam(lr=1e-3, fused=True, capturable=True)" if args.torch_adam else "zhusuan.optim.FlatAdam(lr=1e-3)",
            "discarded_draws": "skipped (zhusuan.skip_discarded_draws)" if skip_discarded else "executed (the package default, as the reference: both draws of the latent, in one launch)",
            "launch_mode": mode,
            "timing": "%d steps in one window, bracketed by synchronize + barrier, max over ranks" % args.steps}
        long_settings = {
            "dense_layers": "zhusuan.Linear / zhusuan.Sequential keep torch.nn.Linear's parameters, names and fp32 GEMMs (forward with "
                            "torch._addmm_activation: the same hipBLASLt solution with the ReLU in its epilogue); per layer one launch of this "
                            "package forms the activation's backward and the bias gradient (extra_configs.c3_torch_linear: torch.nn modules)",
            "mlp_gemm_selection": "PyTorch TunableOp times the fp32 hipBLASLt / rocBLAS solutions per GEMM shape during warm-up and keeps the "
                                  "fastest (callers' nn.Linear stack, outside the hot path; extra_configs.c3_default_gemm: PyTorch's default)",
            "optimizer": "zhusuan.optim.FlatAdam: torch.optim.Adam's update over flat buckets, one launch per bucket "
                         "(extra_configs.c3_torch_adam: torch's multi-tensor Adam)",
            "discarded_draws": "the reference draws every latent twice per objective evaluation and uses the second draw (bn.py:158 / "
                               "elbo.py:122); both are executed here by default; extra_configs.c3_skip_discarded_draws is the opt-in "
                               "zhusuan.skip_discarded_draws()",
            "reference_example": "extra_configs.c3_reference_example is the reference's example as written: torch.nn modules, "
                                 "torch.optim.Adam(params, lr), PyTorch's default GEMM selection, both draws, an eager Python loop, a new "
                                 "minibatch copied in every step (iwae.py:133-160); ..._graphed is the same with zhusuan.GraphedStep "
                                 "(and capturable=True on the optimizer, which torch requires for capture) and nothing else"}
        out = {
            "metric": baseline_metric(),
            "value": evals_per_step * world * args.steps / elapsed,
            "unit": "ELBO-evals/s",
            "n_gpus": world, "n_ranks_seen": dist.get_world_size() if dist.is_initialized() else 1,
            "replicas_in_sync": None if replicas is None else replicas["in_sync"],
            "collective_library": collective_library(share_device) if dist.is_initialized() else None,
            "collective_path": None if not multi else (
                ("RCCL called directly on the compute stream (own communicator, no event records)" if rccl is not None
                 else "torch.distributed all_reduce (synchronous form, current stream)") +
                ("; the decoder bucket asynchronously on the collective library's stream" if staged else "")),
            **({"same_process": same_process} if same_process else {}),
            "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "trials": len(trials), "timed_seconds_total": float(sum(trials)),
            "higher_is_better": True, "scaling": "strong" if args.strong_scaling else "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": settings,
            "final_loss": final_loss,
            "library": library_record(klib), "env_overrides": env_overrides(),
            **({"test_mode": "ranks share GPU 0 and reduce over gloo (ZS_BENCH_SHARE_DEVICE): control-flow test, NOT a measurement"}
               if share_device else {}),
            "roofline": roof,
        }
        # everything that does not fit a one-line record (the driver keeps the line's scalars): per-kernel tables, trial times, prose
        if args.full:
            full = {"trial_ms_per_step": {"min": 1e3 * min(trials) / args.steps, "median": 1e3 * elapsed / args.steps,
                                          "max": 1e3 * max(trials) / args.steps, "all": [1e3 * t / args.steps for t in trials]},
                    "settings_explained": long_settings, "hip_kernels": per_kernel,
                    "roofline_notes": {"timing": timing, "traffic_source": traffic_source,
                                       "working_set": "%.0f MB per launch: resident in the 256 MiB Infinity Cache between the producer kernel and "
                                                      "this one; hbm_resident holds the streaming kernels on working sets beyond it" % (algo_bytes / 1e6)}}
            iw1f = per_kernel.get("zs_bernoulli_iw_objective_f32")
            if iw1f and "frac_of_hbm_peak" in iw1f:
                roof["iw1_fwd_frac"] = iw1f["frac_of_hbm_peak"]        # the step's forward Bernoulli stream + prior + IW objective, one launch
            k3f = per_kernel.get("zs_bernoulli_logprob_f32") or per_kernel.get("zs_bernoulli_logits_logprob_f32")
            if k3f and "frac_of_hbm_peak" in k3f:
                roof["k3_fwd_frac"] = k3f["frac_of_hbm_peak"]          # (a step that runs K3 forward by itself: its in-step figure)
        extras = args.full and world == 1 and not args.no_extras and not args.force_collective_path
        if extras:
            try:
                full["hbm_resident"] = hb = dict(k1_first, **hbm_resident_kernels(klib, dev))
                # the kernel BASELINE.json's north_star sets its >= 60 % target on: flat scalars in the driver-visible line
                for key, label in (("zs_normal_sample_logprob_f32@1M", "k1_frac_1M"), ("zs_normal_sample_logprob_f32", "k1_frac_4M")):
                    if key in hb:
                        roof[label] = hb[key]["frac_of_hbm_peak"]
                # ... and the same launches after a second of idling (average of the 30: the clock ramps inside them)
                for key, label in (("zs_normal_sample_logprob_f32@1M_cold", "k1_frac_1M_cold"), ("zs_normal_sample_logprob_f32@4M_cold", "k1_frac_4M_cold")):
                    if key in hb:
                        roof[label] = hb[key]["frac_of_hbm_peak_avg"]
                dom = hb.get("zs_bernoulli_logprob_bwd_f32")
                if dom:
                    roof["hbm_resident_frac"] = dom["frac_of_hbm_peak"]       # the Bernoulli backward stream at 831 MB (beyond the cache)
                if "k3_fwd_frac" not in roof and "zs_bernoulli_logprob_f32@config" in hb:
                    roof["k3_fwd_frac"] = hb["zs_bernoulli_logprob_f32@config"]["frac_of_hbm_peak"]      # K3 forward alone, config size
                full["roofline_notes"]["k1"] = (
                    "zs_normal_sample_logprob_f32 (in-kernel Philox4x32-10, K = 50, D = 40) at 1 M / 4.2 M rows: median of 30 back-to-back "
                    "launches, HIP events bound to each dispatch, each size right after 1 - 4 s of the kernel's own launches (VALU-issue "
                    "bound: the shader clock follows the recent load); k1_frac_*_cold: the AVERAGE of the same 30 launches right after one "
                    "second of idling (a kernel sweep's condition); bytes per row 4*D + 4 written + 8*D/K read (SURVEY.md 8d)")
            except Exception as e:                                  # noqa: BLE001
                full["hbm_resident"] = {"error": short(e)}
            del model, opt, bucket
            torch.cuda.empty_cache()
            ex = full["extra_configs"] = {}

            def extra(key, name, **kw):
                try:
                    ex[key] = run_single_gpu_config(name, dev, args.steps, args.warmup, **kw)
                except Exception as e:                              # noqa: BLE001
                    ex[key] = {"error": short(e)}
            base = dict(tuned=tuned, torch_adam=args.torch_adam, skip_discarded=skip_discarded, dense=dense)
            # the other single-GPU BASELINE configs, in the headline's settings
            extra("c2", "c2", **base)
            extra("c5", "c5", **base)
            extra("c3_probs" if args.fused_logits else "c3_logits", "c3_probs" if args.fused_logits else "c3_logits", **base)
            # what a user of the reference gets by swapping the import: the example as written, and with only GraphedStep added
            ref = dict(tuned=False, skip_discarded=False, dense="torch", refresh=True)
            extra("c3_reference_example", "c3_probs", torch_adam="reference", eager=True, device_rng=False, **ref)
            extra("c3_reference_example_graphed", "c3_probs", torch_adam="reference_capturable", **ref)
            extra("c5_reference_example", "c5", torch_adam="reference", eager=True, device_rng=False, **ref)
            extra("c5_reference_example_graphed", "c5", torch_adam="reference_capturable", **ref)
            # the headline's settings on a NEW minibatch every replay (GraphedStep(inputs=...): a device-to-device copy of the
            # next resident batch in front of each graph launch) -- the reference's loop never trains twice on one batch
            # (iwae.py:151-160)
            extra("c3_refresh", "c3", fused_logits=args.fused_logits, refresh=True, **base)
            # the launch-bound configs with FOUR steps recorded per graph (zhusuan.GraphedStep(steps_per_replay=4)): the idle
            # time between two graph launches is 13 % of the BNN step, 3.5 % of the VAE step, 1 % of the headline step
            extra("c5_4_steps_per_graph", "c5", steps_per_replay=4, **base)
            extra("c2_4_steps_per_graph", "c2", steps_per_replay=4, **base)
            extra("c3_4_steps_per_graph", "c3", fused_logits=args.fused_logits, steps_per_replay=4, **base)
            # the headline's settings launched eagerly from Python (no graph), one resident minibatch
            extra("c3_eager", "c3", eager=True, fused_logits=args.fused_logits, **base)
            extra("c3_eager_torch_linear", "c3", eager=True, fused_logits=args.fused_logits, **dict(base, dense="torch"))
            extra("c5_eager", "c5", eager=True, **base)
            # the reference examples' own default shapes (iwae.py:126,131; bnn_vi.py:116-118), headline settings
            extra("iwae_default", "iwae_default", **base)
            extra("bnn_default", "bnn_default", **base)
            # the objective alone (SURVEY.md 8d metric (i)): forward under no_grad, no backward, no optimizer
            extra("c3_forward_only", "c3", fused_logits=args.fused_logits, forward_only=True, **base)
            # both draws of the latent as two launches (the package makes them in one where the sampling kernel takes the shape)
            extra("c3_one_launch_per_draw", "c3", fused_logits=args.fused_logits, pair_draws=False, **base)
            if not skip_discarded:      # the opt-in that drops the draw the reference discards
                extra("c3_skip_discarded_draws", "c3", fused_logits=args.fused_logits, **dict(base, skip_discarded=True))
            if tuned:                   # PyTorch's default GEMM selection and its multi-tensor Adam (what round 1 measured)
                extra("c3_default_gemm", "c3_probs", tuned=False, torch_adam=True, skip_discarded=skip_discarded)
            if dense == "fused":        # the headline step built from torch.nn modules
                extra("c3_torch_linear", "c3", fused_logits=args.fused_logits, **dict(base, dense="torch"))
            if not args.torch_adam:     # ... and with torch's multi-tensor Adam
                extra("c3_torch_adam", "c3", fused_logits=args.fused_logits, **dict(base, torch_adam=True))
            # the step in its default multi-rank form on ONE rank over RCCL (a child process): SURVEY 8e's fixed cost
            try:
                ex["c3_dp_step_n1"] = dp_step_on_one_rank(args, out["value"])
            except Exception as e:                                  # noqa: BLE001
                ex["c3_dp_step_n1"] = {"error": short(e)}
            out["extra_configs"] = dict((k, ({"ms_per_step": v["ms_per_step"], "value": v["value"]} if "error" not in v else v))
                                        for k, v in ex.items())
            if "error" not in ex["c3_dp_step_n1"]:
                out["extra_configs"]["c3_dp_step_n1"].update(
                    vs_headline=ex["c3_dp_step_n1"]["vs_headline"], same_process_ratio=ex["c3_dp_step_n1"]["same_process_ratio"],
                    extra_us_per_step=ex["c3_dp_step_n1"]["extra_us_per_step"],
                    collective_library=ex["c3_dp_step_n1"]["collective_library"])
            if "error" not in ex.get("c3_refresh", {"error": 1}):
                # how far a new minibatch per step is from the headline (same settings, same box, same run)
                out["extra_configs"]["c3_refresh"]["vs_headline"] = ex["c3_refresh"]["value"] / out["value"]
        if args.full and world == 1 and not args.no_cpu_baseline:
            cb = cpu_baseline("c3")
            full["cpu_baseline"] = cb
            out["cpu_baseline"] = {"value": cb["value"], "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"],
                                   "sample": cb["sample"], "ms_per_step": cb["ms_per_step"], "one_thread_value": cb["one_thread"]["value"],
                                   "host_cpus_available": cb["host_cpus_available"], "cpu_model": cb["cpu_model"],
                                   "fwd_bwd_only_value": cb.get("fwd_bwd_only", {}).get("value")}
            if extras:
                for name, b1, b2 in (("c2", 2.5, 2.0), ("c5", 2.0, 1.5)):
                    if "error" not in full["extra_configs"].get(name, {"error": 1}):
                        c = cpu_baseline(name, budget_s=b1, one_thread_budget_s=b2, max_steps=2000, fwd_bwd_budget_s=0)
                        full["extra_configs"][name]["cpu_baseline"] = c
                        out["extra_configs"][name]["cpu_value"] = c["value"]
        if args.full:
            try:
                with open(args.full_record, "w") as f:
                    json.dump(dict(out, **full), f, indent=1)
                out["full_record"] = os.path.relpath(args.full_record, ROOT) if args.full_record.startswith(ROOT) else args.full_record
            except OSError as e:
                out["full_record"] = "not written: %r" % (e,)
        print(fit_line(out), flush=True)
    if wd is not None:
        wd.kick("shutdown")
    if rccl is not None:
        rccl.close()
    if dist.is_initialized():
        dist.destroy_process_group()
    if wd is not None:
        wd.stop()


if __name__ == "__main__":
    main()
