#!/usr/bin/env python3
"""Headline benchmark: VQ-IMG 256x256 images/s (recon + VQ, fwd + bwd + Adam) on N MI355X.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

--workload vq (default, BASELINE.json's metric): one "step" = one pass of the hot path over one per-GPU batch of synthetic
images: ``rec, q = VQBASE(x); (|x-rec|.mean() + q).backward(); Adam.step()`` on the model block of the reference's
conf/img_config.yaml (BASELINE configs[1]: VQ-IMG 256x256, codebook 8192, per-GPU batch 32, bf16 activations, fp32 accumulate).
Inputs are resident in HBM before the timed region.  (Since round 6 each layer's weight gradient is issued on a second HIP stream beside its
GroupNorm backward passes -- mas_hip.ops, MAS_WGRAD_STREAM -- and this file defaults GPU_MAX_HW_QUEUES=8 so that RCCL's streams leave it a
hardware queue of its own; the timed region still ends with a device-wide synchronize.)  N > 1: one process per GPU, the reference's own data-parallel scheme
(train.py:24,32: NCCL==RCCL process group + bucketed gradient all-reduce overlapped with backward; SyncBatchNorm's statistics
all-gather), weak scaling (per-GPU batch fixed).

--workload transformer (BASELINE configs[3]): MakeAScene 24L / 1024d / 16 heads over 256 text + 256 seg + 1024 image tokens,
fwd + bwd of the cross-entropy on the image tokens (train.py:150-152) + Adam, bf16 autocast for the library GEMMs, tokens/s.
--workload e2e (BASELINE configs[4]): frozen VQ-SEG + VQ-IMG encode -> tokens -> the same transformer step, samples/s.

A plain run sets up, warms up, times --steps steps, writes the last step's outputs if --dump-outputs DIR is given, and prints the result
line (metric, value, unit, higher_is_better, dtype, ms_per_step and the run's configuration).  --dump-outputs DIR: what the timed path
returned in its last timed step, as DIR/<name>.npy (float32 / float64, 64 MB at most; seeded fixed samples of the larger arrays), from inputs
that are identical from run to run with the same arguments -- two builds compare output for output.

--full adds everything beyond the headline figure.  Rank 0 prints ONE JSON line; with --full it also carries
  "roofline":     the dominant kernel timed live with HIP events on the launch stream inside the timed steps, against the bf16
                  MFMA peak (vq: the 3x3 128->128 conv at 256^2, fwd + dgrad launches, per loader population and launch-weighted
                  -- in training every launch is prologue-free since round 3; transformer / e2e: the causal-attention forward
                  kernel); "mfma_only_floor_ms": the same kernel with everything but MFMAs and LDS reads compiled out (committed);
                  "traffic" / "traffic_over_algorithmic": fabric-side bytes per launch of that kernel INSIDE the step, and
                  "step_traffic_bytes" / "step_traffic_over_algorithmic" / "step_traffic_groupnorm_share": what a whole step moves -- both from the
                  committed rocprofv3 --pmc passes over this very command (tools/step_traffic.sh -> profiles/r06_step_traffic.json; a
                  profiled run cannot also be the timed one);
  "encoder_stack": Encoder.forward of the benched batch timed on its own after the timed steps, against the HBM and MFMA rooflines;
  "cpu_baseline": the reference itself where MAS_REFERENCE_ROOT names a checkout of it (kind "reference"), else the CPU
                  oracle (oracle/vq_oracle.py, a port of the reference's arithmetic: kind "port"), timed
                  on this host's cores on a bounded sample (rank 0, N=1, vq workload only);
  "also":         (vq workload, N=1) compact results of short `--workload transformer` and `--workload e2e` runs (BASELINE configs
                  4 and 5) made right after the headline measurement, so that they carry the same driver clock; --no-also skips them.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: what RCCL / cross-process device memory needs on this driver
# eight HIP hardware queues instead of four: RCCL's streams otherwise leave the weight-gradient side stream on the compute stream's queue
# (mas_hip/__init__.py sets the same default; here it is set before anything can have touched the HIP runtime)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "make-a-scene_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

IMG_CFG = dict(ddconfig=dict(z_channels=256, in_channels=3, out_channels=3, channels=[128, 128, 128, 256, 512, 512],
                             num_res_blocks=2, resolution=512, attn_resolutions=[32], dropout=0.0),
               n_embed=8192, embed_dim=256, init_steps=3000, reservoir_size=12500)   # reference conf/img_config.yaml:19-34
SEG_CFG = dict(ddconfig=dict(z_channels=256, in_channels=159, out_channels=159, channels=[128, 128, 128, 256, 512, 512],
                             num_res_blocks=2, resolution=512, attn_resolutions=[32], dropout=0.0),
               n_embed=256, embed_dim=256, init_steps=3000, reservoir_size=12500)    # conf/seg_config.yaml:13-32
TR_CFG = dict(num_layers=24, hidden_dim=1024, num_attn_heads=16, image_vocab_size=8192, seg_vocab_size=256,
              text_vocab_size=49408 + 256, image_tokens_per_dim=32, seg_tokens_per_dim=16, text_length=256)
PEAK_BF16_TFLOPS = 2500.0      # dense MFMA bf16 peak of the MI355X (vendor figure)
# what v_mfma_f32_32x32x16_bf16 from registers alone sustains on RANDOM bf16 operands on this part: the package power limit holds such a
# loop at 1.865 GHz (constant operands: 2477 TFLOP/s at 2.386 GHz) -- measured, profiles/r05_energy_budget.txt (tools/probes/mfma_power.hip)
RANDOM_DATA_MFMA_CEILING_TFLOPS = 1890.0
PEAK_HBM_GBS = 8000.0
FWD_BWD_GFLOP_PER_IMG = 1337.53     # SURVEY.md section 8(d), counted on the reference with torch flop_counter
TR_FWD_GFLOP_PER_SAMPLE = 1185.4    # full S x S attention count


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15,
                    help="untimed steps; the first ~1 s of load on a cold MI355X runs 5-8 %% slower (clock ramp), so the default covers it")
    ap.add_argument("--workload", default="vq", choices=["vq", "transformer", "e2e"])
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (0 = the BASELINE config: vq 32, transformer 8, e2e 64)")
    ap.add_argument("--micro-batch", type=int, default=16, help="e2e: gradient-accumulation micro-batch (the reference accumulates too)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--dp", default="mas", choices=["mas", "ddp"],
                    help="N>1 gradient averaging: mas_hip.dp.GradReducer (default) or torch DistributedDataParallel")
    ap.add_argument("--grad-dtype", default="fp32", choices=["fp32", "bf16"],
                    help="N>1 with --dp mas: the type the gradient buckets cross the links in (bf16: 190 MB instead of 381 MB per VQ-IMG step; "
                         "A/B knob for the first multi-GPU run, off by default)")
    ap.add_argument("--optimizer", default="mas", choices=["mas", "torch", "torch-default"],
                    help="mas: mas_hip.optim.Adam (the same update as torch.optim.Adam, every parameter in one launch; tests/test_gpu_adam.py); "
                         "torch: torch.optim.Adam(fused=True); torch-default: torch.optim.Adam(params, lr, betas) exactly as the reference's "
                         "train.py:61 constructs it (torch's default foreach implementation)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: roofline / clock / traffic figures, the encoder stack, "
                         "the CPU baseline and (vq, N=1) the short transformer / e2e runs under 'also'; the --no-* options below apply to it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path returned in its last timed step to DIR/<name>.npy (float32 / float64, <= 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline-batch", type=int, default=2)
    ap.add_argument("--cpu-baseline-all-cores", action="store_true",
                    help="also time the CPU oracle on ALL host hardware threads (BASELINE.md section 3's literal recipe; off by default: "
                         "277 s per step was measured with 256 threads in round 1, i.e. nothing finishes inside a bench run)")
    ap.add_argument("--no-encoder-stack", action="store_true", help="skip the Encoder.forward line (kernel traces of the step alone)")
    ap.add_argument("--no-also", action="store_true",
                    help="vq workload at N=1: skip the short runs of the transformer / e2e workloads whose results the line carries under 'also'")
    return ap.parse_args()


# --------------------------------------------------------------------------------------------------------------------
# CPU baseline (vq workload)
# --------------------------------------------------------------------------------------------------------------------
def _reference_root():
    """the reference checkout MAS_REFERENCE_ROOT names, if it holds one"""
    r = os.environ.get("MAS_REFERENCE_ROOT")
    if r and os.path.isfile(os.path.join(r, "models", "vqvae.py")):
        return r
    return None


def _cpu_baseline_worker_reference(batch, threads, timed, ref_root):
    """child process: the REFERENCE ITSELF (imported unmodified from `ref_root`, SURVEY 8(c)'s recipe: the one absent third-party
    import, fast_pytorch_kmeans, is stubbed -- the k-means branch is not entered) on this host's cores: BASELINE.md section 3"""
    import types
    for p_ in [p_ for p_ in sys.path if os.path.isdir(os.path.join(p_ or ".", "models")) and os.path.abspath(p_ or ".") != os.path.abspath(ref_root)]:
        sys.path.remove(p_)                         # `models` must resolve to the reference's package, not to ours
    sys.path.insert(0, ref_root)
    stub = types.ModuleType("fast_pytorch_kmeans")
    stub.KMeans = object
    sys.modules["fast_pytorch_kmeans"] = stub
    from models import VQBASE
    assert os.path.abspath(sys.modules["models"].__file__).startswith(os.path.abspath(ref_root))
    torch.set_num_threads(threads)
    torch.manual_seed(0)
    model = VQBASE(**IMG_CFG).train()
    with torch.no_grad():
        model.quantize.embedding.weight.normal_(0.0, 1.0)
    model.quantize.q_counter = model.quantize.q_re_end
    x = torch.rand(batch, 3, 256, 256, generator=torch.Generator().manual_seed(0))

    def step():
        model.zero_grad(set_to_none=True)
        rec, q = model(x)
        ((x - rec).abs().mean() + q).backward()

    step()
    for _ in range(timed):
        t0 = time.perf_counter()
        step()
        print("CPU_BASELINE_SECONDS", time.perf_counter() - t0, flush=True)


def _cpu_baseline_worker(batch, threads, timed):
    """child process: prints the seconds of each timed CPU-oracle fwd+bwd step"""
    from oracle import vq_oracle as O
    torch.set_num_threads(threads)
    sd = O.synth_state_dict(IMG_CFG["ddconfig"], IMG_CFG["n_embed"], IMG_CFG["embed_dim"], seed=0)
    for v in sd.values():
        if v.is_floating_point():
            v.requires_grad_(True)
    x = O.synth_image_batch(batch, 3, 256, seed=0)

    def step():
        for v in sd.values():
            v.grad = None
        dec, qq, _, _ = O.vqbase_forward(sd, x, IMG_CFG["ddconfig"], training=True)
        O.recon_vq_loss(x, dec, qq).backward()

    step()                                      # warm-up (allocator, oneDNN primitive cache)
    for _ in range(timed):
        t0 = time.perf_counter()
        step()
        print("CPU_BASELINE_SECONDS", time.perf_counter() - t0, flush=True)


def _physical_cores():
    """distinct (physical id, core id) pairs of /proc/cpuinfo (hardware threads / SMT siblings collapse), or None"""
    try:
        cores, phys, core = set(), None, None
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("physical id"):
                    phys = line.split(":")[1].strip()
                elif line.startswith("core id"):
                    core = line.split(":")[1].strip()
                elif not line.strip():
                    if phys is not None and core is not None:
                        cores.add((phys, core))
                    phys = core = None
        return len(cores) or None
    except OSError:
        return None


def _run_cpu_worker(batch, threads, timed, budget_s, ref_root=None):
    import subprocess
    secs, note = [], ""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker", str(batch), str(threads), str(timed)]
                           + ([ref_root] if ref_root else []), capture_output=True, text=True, timeout=budget_s)
        txt, err = r.stdout, r.stderr
    except subprocess.TimeoutExpired as e:
        txt = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        err = ""
        note = f" -- stopped at the {budget_s}s budget"
    for line in txt.splitlines():
        if line.startswith("CPU_BASELINE_SECONDS"):
            secs.append(float(line.split()[1]))
    if not secs:
        note += " -- no step finished" + (": " + err[-200:] if err else "")
    return secs, note


def cpu_baseline(batch, budget_s=150, all_cores=False):
    """Times the CPU oracle (fp32 port of the reference's arithmetic; BASELINE.md section 3's recipe: B=2, 1 warm-up + 3 timed
    fwd+bwd steps of rec,q = model(x); (|x-rec|.mean()+q).backward()) in a child process that is killed after `budget_s`
    seconds -- whatever steps finished by then are reported.  Threads are capped at 32: the host of a GPU box has hundreds of
    slow hardware threads and torch-CPU convolutions get SLOWER beyond a few dozen (round 1: 277 s/step with all 256).
    A reported baseline, not the target."""
    host = os.cpu_count() or 1
    threads = min(host, 32)
    timed = 3
    # the reference itself whenever this machine has a checkout of it (kind "reference"); the GPU box has none: the oracle then
    # (kind "port": the same arithmetic restated, oracle/vq_oracle.py)
    ref_root = _reference_root()
    what = f"the reference's VQBASE imported from {ref_root}" if ref_root else "oracle/vq_oracle.py"
    out = {"value": None, "unit": "images/s", "cores": threads, "host_cpus": host, "host_physical_cores": _physical_cores(),
           "kind": "reference" if ref_root else "port",
           "sample": f"{what}, fp32 fwd+bwd, B={batch} x 256x256, 1 warm-up + {timed} timed steps, {threads} threads of "
                     f"{host} host CPUs, torch CPU {torch.__version__}"}
    secs, note = _run_cpu_worker(batch, threads, timed, budget_s, ref_root)
    if ref_root and not secs:                   # the checkout is there but does not run here: fall back to the port and say so
        out["kind"] = "port"
        out["sample"] = out["sample"].replace(what, "oracle/vq_oracle.py") + f" (the reference at {ref_root} did not finish a step{note})"
        secs, note = _run_cpu_worker(batch, threads, timed, budget_s)
    out["sample"] += note
    if secs:
        out["value"] = round(batch * len(secs) / sum(secs), 4)
        out["timed_steps"] = len(secs)
    if all_cores and host > threads:        # BASELINE.md section 3 as written: every host thread (slower than 32 on these hosts: round 1)
        secs2, note2 = _run_cpu_worker(batch, host, 1, budget_s, ref_root if out["kind"] == "reference" else None)
        out["all_cores"] = {"cores": host, "value": round(batch * len(secs2) / sum(secs2), 4) if secs2 else None,
                            "sample": f"same, {host} threads, 1 warm-up + 1 timed step" + note2}
    else:
        out["all_cores"] = {"cores": host, "value": None,
                            "sample": "not run by default (--cpu-baseline-all-cores): with all 256 threads of such a host one B=2 step took 277 s in "
                                      "round 1 (0.007 images/s) -- torch-CPU convolutions slow down beyond a few dozen threads"}
    return out


# --------------------------------------------------------------------------------------------------------------------
# GradReducer + zero_grad: set_to_none=False keeps .grad a view of the flat bucket and lets autograd ADD the next gradient into it (no
# flatten copy, but one in-place add launch per parameter); set_to_none=True hands autograd fresh tensors and the bucket is flattened by
# one batched copy.  A/B at world size 1: profiles/r05_dropin_defaults.txt
_REDUCER_SET_TO_NONE = os.environ.get("MAS_BENCH_REDUCER_SET_TO_NONE", "1") == "1"      # (measured: -1.5 ms per step against the in-place scheme)


def _adam(args, params, **kw):
    """reference train.py:99-103: torch.optim.Adam.  --optimizer mas (default) = the same update from one kernel launch"""
    if getattr(args, "optimizer", "mas") == "mas":
        from mas_hip.optim import Adam
        return Adam(params, **kw)
    if args.optimizer == "torch-default":       # exactly what reference train.py:61 constructs: torch.optim.Adam(params, **cfg) -- the foreach path
        return torch.optim.Adam(params, **kw)
    return torch.optim.Adam(params, fused=True, **kw)


def _step_traffic():
    """The COMMITTED rocprofv3 PMC summary of whole training steps of THIS command (tools/step_traffic.sh: FETCH_SIZE / WRITE_SIZE / request-size
    counters in their own passes over `bench.py --steps 3 --warmup 2`; profiles/r06_step_traffic.{txt,json}) -- a profiled run cannot also
    be the timed one, so the bench line carries the committed figures and says so."""
    try:
        with open(os.path.join(ROOT, "profiles", "r06_step_traffic.json")) as f:
            return json.load(f)
    except Exception:
        return None


def _pmc_traffic():
    """Fabric-side bytes (L2 <-> Infinity Cache / HBM) per launch of the dominant kernel, measured INSIDE the step (round 6; until round 5 a
    kbench back-to-back loop whose inputs partly sat in the Infinity Cache): 2 x FETCH_SIZE (every read request is a 128-byte line fill)
    + WRITE_SIZE, averaged over the 20 launches of the shape per step."""
    st = _step_traffic()
    if st and st.get("dominant_launch"):
        return int(st["dominant_launch"]["hbm_bytes_per_launch"])
    return None


def _encoder_stack(model, x, batch, dtype):
    """The north_star's own target line: the fused conv+GN+SiLU encoder stack (forward) against the
    HBM and MFMA rooflines, from SURVEY.md section 8(d)'s per-image figures (152.34 Melem of
    algorithmic traffic, 152.19 GFLOP).  Timed after the bench region, outside `value`."""
    esz = 2 if dtype == "bf16" else 4
    with torch.no_grad():
        for _ in range(2):
            model.encoder(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 5
        e0.record()
        for _ in range(reps):
            model.encoder(x)
        e1.record()
        e1.synchronize()
    ms = e0.elapsed_time(e1) / reps
    gbs = 152.34e6 * esz * batch / (ms * 1e-3) / 1e9
    tfs = 152.19e9 * batch / (ms * 1e-3) / 1e12
    peak = PEAK_BF16_TFLOPS if dtype == "bf16" else 157.3
    return {"what": "Encoder.forward, all 23 layers, batch %d" % batch, "fwd_ms": round(ms, 3),
            "algorithmic_hbm_gbs": round(gbs, 1), "hbm_frac": round(gbs / PEAK_HBM_GBS, 4),
            "tflops": round(tfs, 1), "mfma_frac": round(tfs / peak, 4), "binding_bound": "mfma",
            "north_star_target_hbm_frac": 0.40}


def _setup_dist(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with torch.distributed.run", file=sys.stderr)
        if world == 1 and args.gpus > 1:
            sys.exit(2)
    if not torch.cuda.is_available():
        print("bench.py needs an MI355X (no CPU fallback for the product path)", file=sys.stderr)
        sys.exit(2)
    # MAS_BENCH_SHARE_GPU=1 + MAS_BENCH_BACKEND=gloo: functional check of the N>1 code path (reducer, SyncBatchNorm
    # exchange, max-over-ranks timing) with several ranks on ONE GPU -- RCCL refuses two ranks per device, gloo does not
    if os.environ.get("MAS_BENCH_SHARE_GPU") == "1":
        local_rank = 0
    backend = os.environ.get("MAS_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    ddp = world > 1 or os.environ.get("MAS_BENCH_FORCE_DDP") == "1"     # the env knob exercises the N>1 code path on one GPU
    if ddp:
        # (rounds 3-4 set MAS_WGRAD_OVERSUB=2 here -- weight-gradient grids at 2 work-groups per CU, so that a CU taken by a co-running RCCL
        #  kernel costs half a round instead of a whole one.  Measured in round 5 at world size 1: +1.8 ms per step, every step (twice the
        #  split-K slabs), against an expected saving of < 1 ms for the 2-4 ms per step a 381 MB all-reduce is in flight.  Off by default;
        #  the knob stays: profiles/r05_dropin_defaults.txt)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if backend == "nccl":
            dist.init_process_group("nccl", init_method="env://", world_size=world, rank=rank, device_id=dev)
        else:
            dist.init_process_group(backend, init_method="env://", world_size=world, rank=rank)
    return world, rank, local_rank, dev, ddp


def _wrap_dp(model, args, ddp, local_rank):
    net, reducer = model, None
    if ddp and args.dp == "ddp":                            # the reference's wrapper (train.py:31-34)
        net = torch.nn.parallel.DistributedDataParallel(model, device_ids=[local_rank], gradient_as_bucket_view=True)
    elif ddp:                                               # same semantics, a few flat buckets instead of per-parameter copies
        from mas_hip.dp import GradReducer
        reducer = GradReducer(model.parameters(), grad_dtype=torch.bfloat16 if args.grad_dtype == "bf16" else None)
    return net, reducer


class _ClockPower:
    """Shader clock and package power of the benched GPU over the timed region, from the amdgpu hwmon files of the card
    the HIP device maps to (matched by PCI address; profiles/r04_clock_power.txt shows the same files per kernel).  A daemon thread
    reads two small sysfs files every 20 ms: no GPU work, no synchronisation.  Everything is None where the files are not readable."""

    def __init__(self, dev):
        import glob
        import threading
        self.rows, self.on, self.files, self._th = [], False, None, None
        try:
            p = torch.cuda.get_device_properties(dev)
            want = "%04x:%02x:%02x" % (getattr(p, "pci_domain_id", 0), p.pci_bus_id, p.pci_device_id)
            for card in glob.glob("/sys/class/drm/card[0-9]*/device"):
                if os.path.basename(os.path.realpath(card)).lower().startswith(want):
                    for hw in glob.glob(os.path.join(card, "hwmon", "hwmon*")):
                        f, w = os.path.join(hw, "freq1_input"), os.path.join(hw, "power1_input")
                        if os.path.exists(f):
                            self.files = (f, w if os.path.exists(w) else os.path.join(hw, "power1_average"))
            if self.files:
                self._th = threading.Thread(target=self._run, daemon=True)
        except Exception:
            self.files = None

    def _run(self):
        while self.on:
            try:
                with open(self.files[0]) as f:
                    hz = int(f.read())
                with open(self.files[1]) as f:
                    uw = int(f.read())
                self.rows.append((hz / 1e6, uw / 1e6))
            except (OSError, ValueError):
                pass
            time.sleep(0.02)

    def start(self):
        if self._th is not None:
            self.on = True
            self._th.start()

    def stop(self):
        self.on = False
        if self._th is not None:
            self._th.join(timeout=1.0)
        if not self.rows:
            return None
        mhz, w = [r[0] for r in self.rows], [r[1] for r in self.rows]
        return {"sustained_clock_mhz": round(sum(mhz) / len(mhz), 0), "min_clock_mhz": round(min(mhz), 0),
                "package_power_w": round(sum(w) / len(w), 0), "max_package_power_w": round(max(w), 0), "samples": len(mhz)}


def _timed(step, args, ddp, dev, on_start=None):
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if ddp:
        dist.barrier()
    torch.cuda.synchronize()
    if on_start:
        on_start(True)
    t0 = time.perf_counter()
    loss = None
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    if ddp:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if on_start:
        on_start(False)
    if ddp:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt, float(loss.detach())


def _replica_spread(model, ddp):
    if not ddp:                                             # replicas must still hold identical weights after the timed steps
        return None
    with torch.no_grad():
        cs = torch.stack([p.detach().double().sum() for p in model.parameters()]).sum().reshape(1)
    lo, hi = cs.clone(), cs.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    return float((hi - lo).item())


def _flush_libc():
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()


def _emit(out):
    """the ONE JSON line, as the last thing on stdout: RCCL prints its version banner through C stdio, which (stdout being a pipe) sits in
    libc's buffer until exit and would otherwise land AFTER this line -- flush libc first"""
    _flush_libc()
    print(json.dumps(out), flush=True)


_DUMP_BYTES = 64 * 2 ** 20
_ARRAY_SAMPLE = 8 * 2 ** 20          # elements of one dumped output at most (a seeded fixed sample of a larger one)
_PARAM_SAMPLE = 2 * 2 ** 20          # parameter elements dumped (seeded fixed sample of all parameters, concatenated in model order)


def _sample(t, k, seed):
    """t flattened, or a seeded fixed sample of up to k of its elements (k draws, repeats dropped, ascending index order) when it has more"""
    import numpy as np
    flat = t.detach().reshape(-1)
    if flat.numel() <= k:
        return flat
    idx = np.unique(np.random.default_rng(seed).integers(0, flat.numel(), size=k))
    return flat[torch.from_numpy(idx).to(flat.device)]


def _dump_outputs(out_dir, arrays, params):
    """--dump-outputs: `arrays` (name -> tensor, the last timed step's outputs; integer tokens are exact in float32) plus the trained
    parameters as a per-parameter float64 sum and a seeded fixed sample, to out_dir/<name>.npy"""
    import numpy as np
    params = [p.detach() for p in params]
    arrays = {k: (_sample(t, _ARRAY_SAMPLE, seed=2 + i) if t.numel() > _ARRAY_SAMPLE else t) for i, (k, t) in enumerate(arrays.items())}
    arrays["param_sums"] = torch.stack([p.double().sum() for p in params])
    arrays["param_sample"] = _sample(torch.cat([p.float().reshape(-1) for p in params]), _PARAM_SAMPLE, seed=1)
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        t = t.detach()
        a = (t if t.dtype == torch.float64 else t.float()).cpu().numpy()
        total += a.nbytes
        if total > _DUMP_BYTES:
            raise RuntimeError(f"--dump-outputs: {total} bytes exceed the {_DUMP_BYTES}-byte budget at '{name}'")
        np.save(os.path.join(out_dir, name + ".npy"), a)


def _par(world, args, ddp):
    return f"dp{world}" + ((" (DistributedDataParallel" if args.dp == "ddp" else " (mas_hip.dp.GradReducer: 128 MiB flat buckets" + (" crossing the links as bf16," if args.grad_dtype == "bf16" else ","))
                           + " RCCL all-reduce overlapped with backward)" if ddp else "")


# --------------------------------------------------------------------------------------------------------------------
# workload: vq (the headline metric)
# --------------------------------------------------------------------------------------------------------------------
def run_vq(args):
    world, rank, local_rank, dev, ddp = _setup_dist(args)
    from mas_hip import ops
    from models import VQBASE
    batch = args.batch or 32
    cdt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    ops.set_compute_dtype(cdt)

    torch.manual_seed(0)                                   # identical replicas (DDP would broadcast anyway)
    model = VQBASE(**IMG_CFG)
    with torch.no_grad():                                  # post-k-means-like codebook scale
        model.quantize.embedding.weight.normal_(0.0, 1.0)
    model = model.to(dev).train()
    model.quantize.q_counter = model.quantize.q_re_end      # steady state: VQ lookup on the path, no warm-up bypass
    net, reducer = _wrap_dp(model, args, ddp, local_rank)
    opt = _adam(args, model.parameters(), lr=5e-6, betas=(0.5, 0.9))                    # conf/img_config.yaml:36-41

    g = torch.Generator(device="cpu").manual_seed(1234 + rank)          # distinct data per rank
    x = torch.rand(batch, 3, 256, 256, generator=g).to(dev)

    # ---- live timing of the dominant kernel (HIP events on the launch stream) -------------
    dom = {"plain": [], "gn_silu": [], "on": False}

    def hook(kind, shape, launch):
        # shape = (n,h,w,cin,ho,wo,cout,ks,stride,act,has_residual)
        if dom["on"] and kind == "conv_fwd" and shape[3] == 128 and shape[6] == 128 and shape[7] == 3 and shape[8] == 1 \
                and shape[4] == 256 and shape[5] == 256 and shape[1] == 256:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            dom["gn_silu" if shape[9] else "plain"].append((e0, e1))
        else:
            launch()

    if args.full:
        ops.set_launch_hook(hook)
    last = {}

    def step():
        rec, q = net(x)
        loss = (x - rec).abs().mean() + q
        loss.backward()
        if reducer is not None:
            reducer.finish()
        opt.step()
        # the reference's own set_to_none behaviour; with the reducer too since round 5 (its buckets are then flattened by one batched copy
        # each -- keeping .grad a view of the bucket made autograd ADD into it: 345 in-place add launches per step, +1.5 ms)
        opt.zero_grad(set_to_none=reducer is None or _REDUCER_SET_TO_NONE)
        if args.dump_outputs:
            last.update(rec=rec.detach(), q_loss=q.detach(), loss=loss.detach())
        return loss

    torch.cuda.reset_peak_memory_stats(dev)
    cp = _ClockPower(dev) if rank == 0 and args.full else None

    def on_start(on):
        dom["on"] = on
        if cp is not None and on:
            cp.start()

    dt, final_loss = _timed(step, args, ddp, dev, on_start=on_start)
    clock_power = cp.stop() if cp is not None else None
    ops.set_launch_hook(None)
    peak_gib = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    spread = _replica_spread(model, ddp)
    if rank == 0 and args.dump_outputs:
        _dump_outputs(args.dump_outputs, last, model.parameters())
        last.clear()

    if rank == 0:
        value = batch * world * args.steps / dt
        out = {
            "metric": "VQ-IMG 256x256 images/sec/node (recon+VQ fwd+bwd)", "value": round(value, 2), "unit": "images/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "VQ-IMG 256x256, codebook 8192x256, conf/img_config.yaml model block (95.2 M params), "
                                   "fwd+bwd of L1+q_loss + Adam step", "per_gpu_batch": batch, "global_batch": batch * world,
                       "parallelism": _par(world, args, ddp) + (" + SyncBatchNorm" if ddp else ""),
                       "optimizer": {"mas": "mas_hip.optim.Adam (one launch; = torch.optim.Adam's update)", "torch": "torch.optim.Adam(fused=True)",
                                     "torch-default": "torch.optim.Adam(params, lr, betas) as reference train.py:61 (foreach)"}[args.optimizer]},
            "final_loss": round(final_loss, 5),
            "replica_weight_checksum_spread": spread,
            "model_tflops_per_gpu": round(value / world * FWD_BWD_GFLOP_PER_IMG / 1e3, 1),
            # allocator high-water mark of the step: the materialised GroupNorm+SiLU tensors (MAS_GN_MATERIALIZE=1) are saved
            # for the weight gradients on top of the GroupNorm inputs -- about +12 GiB at batch 32; MAS_GN_MATERIALIZE=0 trades them
            # for the slower fused loaders ("Memory")
            "peak_memory_gib": round(peak_gib, 2),
        }
        n_ev = len(dom["plain"]) + len(dom["gn_silu"])
        if n_ev:
            px = batch * 256 * 256
            flops = 2.0 * 9 * 128 * 128 * px                 # algorithmic FLOPs of one launch
            esz = 2 if args.dtype == "bf16" else 4
            bytes_ = 2.0 * px * 128 * esz                    # one read of the input, one write of the output
            peak = PEAK_BF16_TFLOPS if args.dtype == "bf16" else 157.3
            pops = {}
            tot_ms = 0.0
            for k in ("plain", "gn_silu"):
                ms = [a.elapsed_time(b) for a, b in dom[k]]
                if ms:
                    tot_ms += sum(ms)
                    avg = sum(ms) / len(ms)
                    pops[k] = {"launches": len(ms), "avg_launch_ms": round(avg, 4), "tflops": round(flops / (avg * 1e-3) / 1e12, 1),
                               "frac": round(flops / (avg * 1e-3) / 1e12 / peak, 4)}
            avg_ms = tot_ms / n_ev                           # launch-weighted over both populations
            ach = flops / (avg_ms * 1e-3) / 1e12
            out["roofline"] = {"kernel": "3x3 stride-1 128->128 conv @256x256: conv3x3_wide_kernel (fwd + dgrad launches of the step; "
                                         "'plain' = prologue-free launches -- since round 3 all of them in training: the GroupNorm+SiLU output is "
                                         "written once by mas_gn_act, MAS_GN_MATERIALIZE=1 --, 'gn_silu' = forwards with the fused loader, "
                                         "MAS_GN_MATERIALIZE=0; the forward launches also carry the next GroupNorm's statistics in their epilogue)",
                               "bound": "mfma", "achieved": round(ach, 1), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                               "traffic": _pmc_traffic(),
                               "traffic_source": "committed rocprofv3 PMC passes over whole steps of this command (profiles/r06_step_traffic.json, tools/"
                                                 "step_traffic.sh): per-launch average of the shape INSIDE the step, 2 x FETCH_SIZE + WRITE_SIZE; not measured by this run",
                               "avg_launch_ms": round(avg_ms, 4), "launches_timed": n_ev, "populations": pops,
                               "algorithmic_gflop_per_launch": round(flops / 1e9, 1),
                               "algorithmic_hbm_gbs": round(bytes_ / (avg_ms * 1e-3) / 1e9, 1),
                               "hbm_frac": round(bytes_ / (avg_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)}
        if args.full and not args.no_encoder_stack:
            out["encoder_stack"] = _encoder_stack(model, x, batch, args.dtype)
        if "roofline" in out:
            st = _step_traffic()
            if st and st.get("per_gpu_batch") == batch:
                # the step's real traffic next to its algorithmic bytes: GroupNorm's passes count zero bytes by SURVEY 8(d)'s
                # rule and move a third of what crosses the fabric; the convolutions fetch ~1.85x their algorithmic bytes (32-channel chunks
                # touch every 128-byte line twice, ~8 us apart, and the second touch misses the XCD's L2 one time in three; split-K slabs)
                out["roofline"]["step_traffic_bytes"] = int(st["step_traffic_bytes"])
                out["roofline"]["step_algorithmic_bytes"] = int(st["algorithmic_bytes"])
                out["roofline"]["step_traffic_over_algorithmic"] = round(st["step_traffic_over_algorithmic"], 2)
                out["roofline"]["step_traffic_groupnorm_share"] = round(st["groupnorm_bytes"] / st["step_traffic_bytes"], 2)
                out["roofline"]["step_traffic_gbs"] = round(st["step_traffic_bytes"] / (dt / args.steps) / 1e9, 1)   # at THIS run's step time
                if out["roofline"].get("traffic") and st.get("dominant_launch"):
                    out["roofline"]["traffic_over_algorithmic"] = round(st["dominant_launch"]["hbm_bytes_per_launch"] / st["dominant_launch"]["algorithmic_bytes"], 2)
            # what this tile design can reach on this silicon: the shipped kernel with everything but its MFMAs and LDS fragment reads
            # compiled out (profiles/r02_wide_store_ablation.txt / DESIGN R2.2: 0.466 ms at the ~1.6 GHz the chip sustains under this
            # load = 1.33 PFLOP/s): the vendor peak `frac` is priced against assumes 2.4 GHz
            out["roofline"]["mfma_only_floor_ms"] = 0.400
            # the whole step's shader clock and package power (hwmon, sampled every 20 ms over the timed region): the convolution kernels
            # run into the ~1.4 kW package cap and the firmware lowers the clock (profiles/r04_clock_power.txt: 1.70-1.76 GHz under the wide
            # kernel); `frac` above is priced against the vendor peak at 2.4 GHz, `frac_of_peak_at_sustained_clock` against the same matrix
            # cores at the clock this step actually sustained
            if clock_power:
                out["roofline"].update(clock_power)
                peak_s = peak * clock_power["sustained_clock_mhz"] / 2400.0
                out["roofline"]["peak_at_sustained_clock"] = round(peak_s, 1)
                out["roofline"]["frac_of_peak_at_sustained_clock"] = round(ach / peak_s, 4)
            else:
                out["roofline"]["sustained_clock_mhz"] = None
            out["roofline"]["mfma_only_floor_source"] = "committed ablation (kbench, MFMA + LDS reads only), not measured by this run"
            # the ceiling of ANY bf16 kernel on real data on this part (a register-only MFMA loop on random operands sits on the power
            # limit at 1.865 GHz): committed measurement, not made by this run
            out["roofline"]["random_data_mfma_ceiling_tflops"] = RANDOM_DATA_MFMA_CEILING_TFLOPS
            out["roofline"]["frac_of_random_data_mfma_ceiling"] = round(ach / RANDOM_DATA_MFMA_CEILING_TFLOPS, 4)
            out["roofline"]["random_data_mfma_ceiling_source"] = "profiles/r05_energy_budget.txt (tools/probes/mfma_power.hip, >= 5 s loops, hwmon-sampled)"
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.cpu_baseline_batch, all_cores=args.cpu_baseline_all_cores)
        if args.full and world == 1 and not args.no_also and os.environ.get("MAS_BENCH_ALSO", "1") == "1":
            del model, net, opt, x                               # free the HBM the other workloads need
            torch.cuda.empty_cache()
            out["also"] = _also_workloads()
        final_line = out
    if ddp:
        _flush_libc()                     # every rank: whatever C-level output it holds goes out BEFORE rank 0's line
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        _emit(final_line)                 # after the process group is gone: nothing of RCCL's can follow the line


def _also_workloads(budget_s=240):
    """BASELINE configs 4 and 5 under the same clock as the headline line: short runs of `--workload transformer` and `--workload e2e`
    as child processes (their own process = their own allocator and TunableOp state), compact results embedded under "also".  They are
    NOT part of `value`; the full lines come from running those workloads directly."""
    import subprocess
    res = {}
    for wl, extra in (("transformer", ["--steps", "12", "--warmup", "6"]), ("e2e", ["--steps", "3", "--warmup", "2"])):
        t0 = time.perf_counter()
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", wl, "--gpus", "1", "--full", "--no-cpu-baseline"] + extra,
                               capture_output=True, text=True, timeout=budget_s)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            d = json.loads(line[-1])
            res[wl] = {"metric": d["metric"], "value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"], "steps": d["steps"],
                       "warmup": d["warmup"], "dtype": d["dtype"], "per_gpu_batch": d["config"]["per_gpu_batch"],
                       "model_tflops_per_gpu": d.get("model_tflops_per_gpu"),
                       "roofline": {k: d["roofline"][k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_ms")}
                       if "roofline" in d else None,
                       "wall_s": round(time.perf_counter() - t0, 1)}
        except Exception as e:                                   # never let a side run break the headline line
            res[wl] = {"error": f"{type(e).__name__}: {str(e)[:200]}", "wall_s": round(time.perf_counter() - t0, 1)}
    return res


# --------------------------------------------------------------------------------------------------------------------
# workloads: transformer (config 4) and e2e (config 5)
# --------------------------------------------------------------------------------------------------------------------
def _library_gemm_selection():
    """The Linear layers are plain library GEMMs (hipBLASLt / rocBLAS through torch).  PyTorch's TunableOp picks, per GEMM shape,
    the fastest of the libraries' own solutions; the selection measured on an MI355X for this workload's 15 shapes is committed
    (make-a-scene_amd/tuning/, +2 % on the step) and only REPLAYED here: no tuning inside a bench run, and a file whose validator
    lines do not match the installed libraries is ignored by TunableOp itself.  MAS_BENCH_TUNABLEOP=0 turns it off."""
    path = os.path.join(ROOT, "make-a-scene_amd", "tuning", "tunableop_gfx950_transformer.csv")
    if os.environ.get("MAS_BENCH_TUNABLEOP", "1") != "1" or not os.path.exists(path):
        return None
    try:
        import torch.cuda.tunable as tunable
        tunable.enable(True)
        tunable.tuning_enable(False)
        tunable.set_filename(path)
        return os.path.basename(path) if tunable.read_file(path) else None
    except Exception as e:                                   # a torch build without TunableOp: library defaults
        print(f"bench.py: TunableOp replay unavailable ({e}); library default GEMM selection", file=sys.stderr)
        return None


def run_transformer(args, e2e):
    world, rank, local_rank, dev, ddp = _setup_dist(args)
    gemm_sel = _library_gemm_selection()
    from mas_hip import ops
    from models import VQBASE
    from models.transformer import MakeAScene
    batch = args.batch or (64 if e2e else 8)
    micro = min(args.micro_batch, batch) if e2e else batch
    if batch % micro:
        raise SystemExit("--batch must be a multiple of --micro-batch")
    cfg = TR_CFG
    S = cfg["text_length"] + cfg["seg_tokens_per_dim"] ** 2 + cfg["image_tokens_per_dim"] ** 2
    torch.manual_seed(0)
    model = MakeAScene(**cfg).to(dev).train()
    net, reducer = _wrap_dp(model, args, ddp, local_rank)
    opt = _adam(args, model.parameters(), lr=1e-4)
    g = torch.Generator(device="cpu").manual_seed(4321 + rank)
    text = torch.randint(1, 49408, (batch, 256), generator=g)
    text[:, 200:] = 0                                                    # zero-padded tail (transformer.py:350-353)
    text = text.to(dev)
    vq_img = vq_seg = images = segs = None
    if e2e:                                                              # frozen stage-1 models produce the tokens inside the step
        ops.set_compute_dtype(torch.bfloat16)
        vq_img = VQBASE(**IMG_CFG).to(dev).eval().requires_grad_(False)
        vq_seg = VQBASE(**SEG_CFG).to(dev).eval().requires_grad_(False)
        with torch.no_grad():
            vq_img.quantize.embedding.weight.normal_(0.0, 1.0)
            vq_seg.quantize.embedding.weight.normal_(0.0, 1.0)
        images = torch.rand(batch, 3, 512, 512, generator=g).to(dev)      # 512x512 -> 32x32 = 1024 image tokens (img_config.yaml: resolution 512)
        segs = torch.rand(batch, 159, 256, 256, generator=g).to(dev)      # soft one-hot-like maps of the 159 classes
    else:
        seg_tok = torch.randint(0, 256, (batch, 256), generator=g).to(dev)
        img_tok = torch.randint(0, 8192, (batch, 1024), generator=g).to(dev)

    att = {"ev": [], "on": False}
    orig = ops._CausalAttention.forward

    def timed_fwd(ctx, qkv, n_heads, cd):
        if not att["on"]:
            return orig(ctx, qkv, n_heads, cd)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = orig(ctx, qkv, n_heads, cd)
        e1.record()
        att["ev"].append((e0, e1, qkv.shape[0]))
        return r

    if args.full:
        ops._CausalAttention.forward = staticmethod(timed_fwd)
    last = {}

    def step():
        from token_data import tokenize_batch
        loss = None
        for m0 in range(0, batch, micro):
            sl = slice(m0, m0 + micro)
            if e2e:
                it, st = tokenize_batch(vq_img, vq_seg, images[sl], segs[sl])
            else:
                it, st = img_tok[sl], seg_tok[sl]
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=args.dtype == "bf16"):
                logits = net(text[sl], st, it)
            loss = torch.nn.functional.cross_entropy(logits.float().reshape(-1, logits.shape[-1]), it.reshape(-1)) * (micro / batch)
            if reducer is not None and m0 + micro < batch:
                with reducer.no_sync():
                    loss.backward()
            else:
                loss.backward()
            if args.dump_outputs and m0 + micro >= batch:     # the step's last micro-batch
                last.update(logits=logits.detach(), loss=loss.detach())
                if e2e:
                    last.update(image_tokens=it.detach(), seg_tokens=st.detach())
        if reducer is not None:
            reducer.finish()
        opt.step()
        opt.zero_grad(set_to_none=True)
        return loss

    dt, final_loss = _timed(step, args, ddp, dev, on_start=lambda on: att.__setitem__("on", on))
    ops._CausalAttention.forward = staticmethod(orig)
    spread = _replica_spread(model, ddp)
    if rank == 0 and args.dump_outputs:
        _dump_outputs(args.dump_outputs, last, model.parameters())
        last.clear()
    if rank == 0:
        samples = batch * world * args.steps
        gf = TR_FWD_GFLOP_PER_SAMPLE * 3
        if e2e:
            out = {"metric": "end-to-end stage-2 samples/sec/node (frozen VQ-SEG + VQ-IMG encode -> AR transformer fwd+bwd+Adam)",
                   "value": round(samples / dt, 2), "unit": "samples/s"}
            wl = (f"BASELINE configs[4]: frozen VQ-IMG (512x512x3) + VQ-SEG (256x256x159) encode -> 1024 + 256 tokens -> MakeAScene 24L/1024d/16h "
                  f"(S={S}) cross-entropy fwd+bwd + Adam, micro-batch {micro} x {batch // micro} accumulation")
        else:
            out = {"metric": "MakeAScene 24L/1024d transformer tokens/sec/node (fwd+bwd+Adam, S=1536)",
                   "value": round(samples * S / dt, 1), "unit": "tokens/s"}
            wl = f"BASELINE configs[3]: MakeAScene 24L/1024d/16 heads (head_dim 64, assumed: SURVEY 8(d)), 256 text + 256 seg + 1024 image tokens"
        out.update({"n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 3),
                    "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
                    "config": {"workload": wl, "per_gpu_batch": batch, "global_batch": batch * world, "parallelism": _par(world, args, ddp),
                               "library_gemm_selection": gemm_sel or "library default"},
                    "final_loss": round(final_loss, 5), "replica_weight_checksum_spread": spread,
                    "model_tflops_per_gpu": round(samples / world / dt * gf / 1e3, 1)})
        if att["ev"]:
            ms = [a.elapsed_time(b) for a, b, _ in att["ev"]]
            nb = att["ev"][0][2]
            avg = sum(ms) / len(ms)
            fl = 4.0 * nb * 16 * S * S * 64 / 2              # causal half of the two S x S x hd products
            ach = fl / (avg * 1e-3) / 1e12
            out["roofline"] = {"kernel": f"attn_causal_fwd_bf16 (B={nb}, H=16, S={S}, hd=64), forward launches of the step (incl. the dtype glue of the autograd wrapper)",
                               "bound": "mfma", "achieved": round(ach, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(ach / PEAK_BF16_TFLOPS, 4), "traffic": None, "avg_launch_ms": round(avg, 4),
                               "launches_timed": len(ms), "algorithmic_gflop_per_launch": round(fl / 1e9, 1)}
        final_line = out
    if ddp:
        _flush_libc()                     # every rank: whatever C-level output it holds goes out BEFORE rank 0's line
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        _emit(final_line)                 # after the process group is gone: nothing of RCCL's can follow the line


def main():
    args = parse()
    if args.workload == "vq":
        run_vq(args)
    else:
        run_transformer(args, e2e=args.workload == "e2e")


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--cpu-baseline-worker":
        if len(sys.argv) > 5:
            _cpu_baseline_worker_reference(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
        else:
            _cpu_baseline_worker(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 1)
    else:
        main()
