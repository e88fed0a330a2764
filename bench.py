#!/usr/bin/env python3
"""Headline benchmark: chord-tokens/s of batched autoregressive generate (BASELINE.json).

One "step" = one pass of the hot path over one batch: video encode + feedback-greedy (G2) decode of
B=32 clips per GPU to T=1024 tokens (+ the all-gather of ids when N>1), inputs resident in HBM.
Workload = BASELINE.json configs[1]: 6+6 layers, d_model=512, H=8, dff=1024, max_sequence_chord=1024,
300-frame synthetic video features (F=1287), random-init procedural weights.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
N>1: one rank per GPU — either started by `python -m torch.distributed.run … bench.py --gpus N …` (the ranks read
RANK / LOCAL_RANK / WORLD_SIZE), or, when no such environment is present, by this script itself: the parent starts the
N ranks as child processes before anything touches a GPU and relays rank 0's line.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps and prints the headline; `--dump-outputs DIR`
writes the chord ids of the last timed step to DIR/chord_ids.npy (float32; inputs and weights are seeded, so two builds can be
compared id for id).  `--full` (one rank) adds the legs below, each a run of its own after the timed steps.

`roofline` is for the dominant kernel (attn_decode_kernel<64>, the K/V-streaming
self-attention of the decode step): algorithmic fp32 K/V bytes / the kernel's launch duration inside the captured step
graph, measured with HIP events on the launch stream; it also carries the cross-attention, the skinny GEMMs, the
step-level figure (`whole_step`, the honest headline of the decode path) and `prefill` = the cross-attention
QK^T/PV kernel of the teacher-forced forward against the fp32 MFMA peak (the north star's named target).
`cpu_baseline` times the CPU oracle (port of the reference's no-KV-cache loop) on the host cores.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "video2music_amd", "lib", "libamt_hip.so")


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32, help="clips per GPU")
    ap.add_argument("--seq", type=int, default=1024, help="target_seq_length = max_sequence_chord")
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--d_model", type=int, default=512)
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's chord ids to DIR/chord_ids.npy")
    ap.add_argument("--full", action="store_true", help="also the roofline, v2_lockstep and cpu_baseline legs")
    ap.add_argument("--no_cpu_baseline", action="store_true", help="with --full: leave out the cpu_baseline leg")
    ap.add_argument("--no_roofline", action="store_true", help="with --full: leave out the roofline and v2_lockstep legs")
    return ap.parse_args()


def ensure_library():
    """The library is a build artefact: build it once if absent.  Ranks started together serialise on a
    file lock, so nobody imports a half-written .so."""
    if os.path.exists(LIB):
        return
    import fcntl
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    with open(os.path.join(os.path.dirname(LIB), ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(LIB):
            subprocess.check_call([os.path.join(ROOT, "video2music_amd", "csrc", "build.sh")], stdout=sys.stderr)


def launch_ranks(args):
    """`python bench.py --gpus N` without a torchrun environment: this parent — which has not imported torch
    and never touches a GPU — starts the N ranks as children of `torch.distributed.run` (one process per GPU,
    RCCL over xGMI), relays rank 0's JSON line and exits with the launcher's status.  No exec."""
    import socket
    ensure_library()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout:
        if ln.lstrip().startswith("{") and '"metric"' in ln:
            line = ln.strip()
        else:
            sys.stderr.write(ln)
    rc = proc.wait()
    if line is not None:
        print(line, flush=True)
    if rc == 0 and line is None:
        sys.stderr.write("bench.py: the ranks finished without printing a result line\n")
        rc = 1
    sys.exit(rc)


if __name__ == "__main__" and "WORLD_SIZE" not in os.environ:
    _a = parse_args()
    if _a.gpus > 1:
        launch_ranks(_a)                                                     # does not return

ensure_library()
import numpy as np                                                           # noqa: E402
import torch                                                                 # noqa: E402
from video2music_amd import dist as vdist                                   # noqa: E402
from video2music_amd import synthetic                                        # noqa: E402
from video2music_amd.model.video_music_transformer import VideoMusicTransformer   # noqa: E402
from video2music_amd.utilities import constants as C                          # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6.3 TB/s achievable
MFMA_F32_PEAK_TFLOPS = 157.3   # dense f32-in / f32-acc matrix peak (same file)


def make_model(cfg, device, seed=0):
    m = VideoMusicTransformer(**cfg).eval()
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=seed).items()}
    m.load_state_dict(sd, strict=False)
    return m.to(device), sd


def cpu_baseline(cfg, sd, T, budget_s=25.0):
    """Per-length cost of one step of the reference loop (full re-forward incl. encoder, no KV
    cache, B=1: model/video_music_transformer.py:1069-1071) integrated over the T-1 steps of a clip.
    Timed with the intra-op thread count that a short calibration finds fastest on this host (8 ... 128 candidates) and, coarser,
    with 8 threads (comparable with the survey container's figures)."""
    from oracle import amt_oracle as O
    prev_threads = torch.get_num_threads()
    feats = synthetic.synthetic_features(1, seed=99)
    f = {k: torch.from_numpy(v) for k, v in feats.items()}

    def per_clip_seconds(threads, lengths, budget):
        torch.set_num_threads(threads)
        rs = np.random.RandomState(0)
        cost = []
        t_start = time.time()
        with torch.no_grad():
            for L in lengths:
                root = torch.from_numpy(rs.randint(1, 13, size=(1, L)))
                attr = torch.from_numpy(rs.randint(1, 14, size=(1, L)))
                reps, best = 0, float("inf")
                while reps < 2 or (reps < 3 and time.time() - t_start < budget * 0.6):
                    t0 = time.perf_counter()
                    O.forward(sd, cfg["num_heads"], root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
                    best = min(best, time.perf_counter() - t0)
                    reps += 1
                cost.append(best)
        return float(np.trapezoid(np.interp(np.arange(1, T), lengths, cost)))

    # thread count: calibrated here, not assumed -- one forward at L = T/2 per candidate (profiles/r03_cpu_baseline_thread_sweep.json
    # is the same sweep recorded at L = 512 on the GPU box); the best candidate is the baseline's `cores`
    ncpu = os.cpu_count() or 1
    cands = [n for n in (8, 16, 32, 64, 128) if n <= ncpu] or [ncpu]
    calib = {}
    rs = np.random.RandomState(1)
    Lc = max(T // 2, 1)                    # the mean length of the integrated loop (short lengths favour more threads than the sample does)
    root = torch.from_numpy(rs.randint(1, 13, size=(1, Lc)))
    attr = torch.from_numpy(rs.randint(1, 14, size=(1, Lc)))
    with torch.no_grad():
        for n in cands:
            torch.set_num_threads(n)
            best = float("inf")
            for _ in range(2):
                t0 = time.perf_counter()
                O.forward(sd, cfg["num_heads"], root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])
                best = min(best, time.perf_counter() - t0)
            calib[n] = best
    best_s = min(calib.values())
    threads = min(n for n, v in calib.items() if v <= 1.05 * best_s)        # within 5 % of the best: the fewer threads
    lengths = sorted({1, T // 16, T // 8, T // 4, (3 * T) // 8, T // 2, (5 * T) // 8, (3 * T) // 4, (7 * T) // 8, T - 1})
    per_clip = per_clip_seconds(threads, lengths, budget_s)
    coarse = sorted({1, T // 4, T // 2, (3 * T) // 4, T - 1})
    per_clip8 = per_clip_seconds(min(8, ncpu), coarse, budget_s * 0.5)
    torch.set_num_threads(prev_threads)
    return {"value": round((T - 1) / per_clip, 3), "unit": "chord-tokens/s", "cores": threads, "kind": "port",
            "sample": f"oracle forward (no KV cache, encoder re-run, B=1) timed at L={lengths} (best of 2-3), "
                      f"integrated over the {T - 1} steps of one clip = {per_clip:.1f} s/clip; clips run sequentially",
            "value_8_threads": round((T - 1) / per_clip8, 3),
            "sample_8_threads": f"same, {min(8, ncpu)} threads, L={coarse} (best of 2): {per_clip8:.1f} s/clip",
            "thread_calibration_s_per_forward": {str(n): round(v, 4) for n, v in calib.items()},
            "thread_calibration": f"one oracle forward at L={Lc} per candidate thread count (best of 2); `cores` = the fewest threads within 5 % of the fastest",
            "host_cpus": ncpu}


def _sha256(path):
    import hashlib
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


PMC_PROFILE = os.path.join(ROOT, "profiles", "r03_pmc_decode_step.json")
PMC_KERNELS = {            # kind -> (source file whose sha gates the figure, kernel-name test)
    "self_attn": ("attn_decode.hip", lambda k: k.startswith("attn_decode_kernel<64, true")),
    "cross_attn": ("attn_decode.hip", lambda k: k.startswith("attn_decode_kernel<64, false")),
    "decode_gemm": ("decode_gemm.hip", lambda k: k.startswith("decode_gemm_kernel<")),
}


def pmc_traffic(kind, shape_ok=True, algorithmic_bytes=None):
    """HBM-side bytes per launch of a decode-step kernel class from the committed PMC passes (tools/gpu_pmc_step.sh: rocprofv3 --pmc
    FETCH_SIZE and --pmc WRITE_SIZE in separate passes -- the skinny GEMMs inside the real captured step, the attention kernels
    through tools/pmc_attn.py over the positions of a T = 1024 generate; FETCH_SIZE doubled per the gfx950 correction of
    MI355X_MICROARCH.md; launch-weighted mean over the kernel's variants).
    Counters cannot be read from inside bench.py, so the figure is reported only while the kernel's source file is byte-identical
    to the one the passes were collected on (sha256 recorded in the profile) and this run has the profile's shape; otherwise null."""
    src_name, match = PMC_KERNELS[kind]
    if not shape_ok:
        return None, "the committed PMC passes were collected at config 2's shape (32 clips, T = 1024, d_model 512) only"
    src = os.path.join(ROOT, "video2music_amd", "csrc", src_name)
    if not (os.path.exists(PMC_PROFILE) and os.path.exists(src)):
        return None, "no committed PMC pass"
    prof = json.load(open(PMC_PROFILE))
    if prof.get("kernel_source_sha256", {}).get(src_name) != _sha256(src):
        return None, f"profiles/r03_pmc_decode_step.json was collected on another version of {src_name}"
    rows = [v for k, v in prof["kernels"].items() if match(k)]
    n = sum(r["dispatches"] for r in rows)
    if not n:
        return None, "kernel not in the committed PMC pass"
    src_note = "profiles/r03_pmc_decode_step.json (rocprofv3 --pmc passes on this kernel source; launch-weighted mean"
    if algorithmic_bytes is not None:      # attention: the pass covers every 8th position; its traffic / algorithmic ratio scaled to this run's bytes
        ratio = sum(r["traffic_bytes_per_launch"] * r["dispatches"] for r in rows) / sum(r["algorithmic_bytes_per_launch"] * r["dispatches"] for r in rows)
        return round(ratio * algorithmic_bytes), src_note + ", traffic / algorithmic ratio scaled to this run's bytes)"
    return round(sum(r["traffic_bytes_per_launch"] * r["dispatches"] for r in rows) / n), src_note + ")"


def prefill_roofline(B, L, S, H, hd, device, reps=20):
    """North-star MFMA figure: the cross-attention prefill kernel (attn_prefill_kernel<64,false>, QK^T + PV of the teacher-forced
    forward, model/rpr.py:62-63) at config 2's shape, timed with HIP events on the launch stream: 4*B*L*S*d flop per launch
    against the dense fp32 MFMA peak (157.3 TFLOP/s, MI355X_MICROARCH.md)."""
    from video2music_amd import _lib
    d = H * hd
    q = torch.randn(B, L, d, device=device) * 0.1
    k = torch.randn(B, S, d, device=device)
    v = torch.randn(B, S, d, device=device)
    o = torch.empty(B, L, d, device=device)

    def run():
        _lib.call("amt_cross_attn_fwd", _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o), B, H, L, S, hd, 0, _lib.stream_ptr())

    # this leg runs right behind the latency-bound decode legs: the first launches of a dense kernel see the clocks of an almost
    # idle chip, so warm up with as many launches as are timed and keep the better of two timed rounds
    for _ in range(reps):
        run()
    us = float("inf")
    for _ in range(2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            run()
        b.record()
        torch.cuda.synchronize()
        us = min(us, 1e3 * a.elapsed_time(b) / reps)
    flop = 4.0 * B * L * S * d
    return {"bound": "mfma", "kernel": "attn_prefill_kernel<64, false> (cross-attention QK^T + PV of the teacher-forced forward)",
            "shape": f"B={B} L={L} S={S} H={H} hd={hd} (grid (2048,8,32)/256... one launch per decoder layer of the config-2 forward)",
            "flop_per_launch": flop, "avg_launch_us": round(us, 2), "achieved": round(flop / us / 1e6, 2), "peak": MFMA_F32_PEAK_TFLOPS,
            "unit": "TFLOP/s", "frac": round(flop / us / 1e6 / MFMA_F32_PEAK_TFLOPS, 4), "dtype": "f32 in / f32 accumulate (v_mfma_f32_32x32x2_f32)",
            "measured": f"HIP events on the launch stream around {reps} back-to-back launches of the operator entry point (same kernel, "
                        f"same grid as the forward's), after {reps} warm-up launches, better of two rounds"}


def forward_leg(model, f, B, T, cfg, reps=5):
    """SURVEY.md §8(d) "also report the prefill forward separately": the teacher-forced forward of the same configuration
    (video encode + 6 decoder layers over B x T chord positions, model/video_music_transformer.py:913-1044) — the MFMA-bound
    side of the path; it is also what the reference's beam=1 branch (top-1 without feedback) costs in ONE call."""
    rs = np.random.RandomState(0)
    dev = f["semantic"].device
    root = torch.from_numpy(rs.randint(1, 13, size=(B, T))).to(dev)
    attr = torch.from_numpy(rs.randint(1, 14, size=(B, T))).to(dev)

    def run():
        model(root, root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])

    with torch.no_grad():
        for _ in range(2):
            run()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            run()
        b.record()
        torch.cuda.synchronize()
    ms = a.elapsed_time(b) / reps
    d, dff, nl, S, F = cfg["d_model"], cfg["dim_feedforward"], cfg["n_layers"], 300, cfg["total_vf_dim"]
    # dense-equivalent flop of the products the forward launches (causal self-attention counted on its visible half)
    enc = B * S * (2 * F * d + nl * (8 * d * d + 4 * d * dff + 4 * S * d))
    dec = B * T * nl * (8 * d * d + 4 * d * d + 4 * d * dff + 4 * S * d + 2 * T * d + T * d) + B * S * nl * 4 * d * d + B * T * 2 * d * 159
    return {"ms": round(ms, 3), "token_positions_per_s": round(B * T / ms * 1e3), "gflop": round((enc + dec) / 1e9, 1),
            "achieved": round((enc + dec) / ms / 1e9, 2), "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round((enc + dec) / ms / 1e9 / MFMA_F32_PEAK_TFLOPS, 4), "shape": f"B={B} L={T} S={S}",
            "flop_model": "2*m*n*k of every product of the encode + decoder forward; causal self-attention (QK^T, Q.Er, PV) counted on the "
                          "visible half: 2*L*d per position for QK^T+PV and L*d for the relative term Q.Er^T",
            "measured": f"HIP events around {reps} forwards (encode included) after 2 warm-up calls"}


def roofline(model, f, prim, B, T, cfg, headline_generate_ms=None):
    """Roofline of the decode step's kernels.

    Dominant kernel = the K/V-streaming relative-position self-attention.  Two measurements of its launch duration:
      * in the captured step graph (what the kernel costs the step): (generate ms - generate ms with the kernel left out of the
        graph) / launches, median of 3 interleaved rounds, HIP events on the launch stream around whole generates.  `achieved`
        and `frac` are computed from THIS figure: it includes the kernel boundary and is the conservative one;
      * HIP event pair around every launch of an eager replay of the same generate (amt_generate_profile), reported as
        `event_pair` both raw and minus the cost of an empty pair.  rocprofv3's kernel-trace average (profiles/) lies between the two.
    """
    with torch.no_grad():
        _, st = model.generate_profile(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], *prim,
                                       target_seq_length=T)

        def timed(mask):
            model._debug_set_skip(mask)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            model.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], *prim,
                                 target_seq_length=T, beam=0, sampler="argmax")
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)

        # The three variants are timed on the chain with ONE launch per kernel class and step (sampling head as its own launch):
        # the shipped graph folds the head into the next step's first self-attention (30 launches per step), which would put a
        # different kernel into the `full` variant than the ones left out of the other two
        model.set_option("fuse_sampling_head", 0)
        for m in (0, 1, 2):
            timed(m)                                         # graph capture / warm-up per variant
        rounds = [[timed(m) for m in (0, 1, 2)] for _ in range(3)]
        model._debug_set_skip(0)
        model.set_option("fuse_sampling_head", 1)
    empty_us = 1e3 * st["empty_event_pair"]["ms"] / st["empty_event_pair"]["launches"]

    def raw_us(k):
        return 1e3 * st[k]["ms"] / st[k]["launches"]

    def ev(k, nbytes=None):
        raw, cor = raw_us(k), max(raw_us(k) - empty_us, 1e-3)
        o = {"avg_launch_us_raw": round(raw, 3), "avg_launch_us_minus_empty_pair": round(cor, 3)}
        if nbytes:
            o["GBps_minus_empty_pair"] = round(nbytes / cor / 1e3, 1)
        return o

    full, no_self, no_cross = (float(np.median([r[i] for r in rounds])) for i in range(3))
    n = st["self_attn_decode"]["launches"]
    self_bytes = st["self_attn_decode"]["bytes"] / n
    cross_bytes = st["cross_attn_decode"]["bytes"] / n
    self_us, cross_us = 1e3 * (full - no_self) / n, 1e3 * (full - no_cross) / n
    steps = T - 1
    step_us = 1e3 * full / steps
    d, dff, nl = cfg["d_model"], cfg["dim_feedforward"], cfg["n_layers"]
    # the skinny GEMMs: packed weights read per launch (folded chain: [Wo | W'.Wo, W'] etc.), 3 launches per layer
    gemm_bytes = (nl * 3 * d * d + nl * (d * d + 2 * d * dff) + nl * d * dff + (nl - 1) * 3 * d * (dff + d) + 160 * (dff + d)) * 4 / (3 * nl)
    n_gemm = st["decode_gemm"]["launches"] / steps
    sample_us = max(raw_us("sample") - empty_us, 0.0)
    gemm_in_chain_us = (step_us - nl * (self_us + cross_us) - sample_us) / max(n_gemm, 1)
    if gemm_in_chain_us <= 0.05:                 # a difference of timings: at small shapes it can come out at or below zero
        gemm_in_chain_us = None

    def rate(nbytes, us):
        return (None, None) if not us else (round(nbytes / us / 1e3, 1), round(nbytes / us / 1e3 / HBM_PEAK_GBS, 4))
    shape_ok = B == 32 and d == 512 and cfg["num_heads"] == 8 and nl == 6
    traffic, traffic_src = pmc_traffic("self_attn", shape_ok, self_bytes)
    return {
        "bound": "hbm", "kernel": "attn_decode_kernel<64, true, true, {0,2}, 2> (relative-position self-attention, decode step; FOLD 2 in layers 1-5)",
        "achieved": round(self_bytes / self_us / 1e3, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": round(self_bytes / self_us / 1e3 / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
        "launches": n, "avg_launch_us": round(self_us, 3), "algorithmic_bytes_per_launch": round(self_bytes),
        "measured": "in the captured step graph: (generate ms - generate ms with the kernel left out of the graph) / launches, HIP events "
                    "on the launch stream, median of 3 interleaved rounds; includes the kernel boundary",
        "generate_ms": {"full": round(full, 2), "without_self_attn": round(no_self, 2), "without_cross_attn": round(no_cross, 2),
                        "note": "31-launch chain (sampling head as its own launch); the headline runs the 30-launch chain"},
        "event_pair": dict(ev("self_attn_decode", self_bytes), empty_pair_us=round(empty_us, 2),
                           method="HIP event pair on the launch stream around every launch of an eager replay of one full generate"),
        "cross_attn": {"kernel": "attn_decode_kernel<64, false, true, 1, 2> (cross-attention over video K/V, decode step)",
                       "algorithmic_bytes_per_launch": round(cross_bytes), "avg_launch_us": round(cross_us, 3),
                       "achieved": round(cross_bytes / cross_us / 1e3, 1), "frac": round(cross_bytes / cross_us / 1e3 / HBM_PEAK_GBS, 4),
                       "traffic": pmc_traffic("cross_attn", shape_ok, cross_bytes)[0], "event_pair": ev("cross_attn_decode", cross_bytes)},
        "decode_gemm": {"kernel": "decode_gemm_kernel<4,true,0> (G1, G2) and <6,true,2> (G3): weight-streaming skinny GEMMs, 18 launches per step",
                        "packed_weight_bytes_per_launch": round(gemm_bytes),
                        "avg_launch_us": None if gemm_in_chain_us is None else round(gemm_in_chain_us, 3),
                        "achieved": rate(gemm_bytes, gemm_in_chain_us)[0], "frac": rate(gemm_bytes, gemm_in_chain_us)[1],
                        "traffic": pmc_traffic("decode_gemm", shape_ok)[0], "traffic_source": pmc_traffic("decode_gemm", shape_ok)[1],
                        "measured": "in the chain: (step us - attention launches - sampling head) / GEMM launches; latency-bound "
                                    "(profiles/r02_skinny_gemm_timeline_before.txt; wave-cycle split in profiles/r03_pmc_decode_step.json)",
                        "event_pair": ev("decode_gemm", gemm_bytes)},
        "sample_event_pair": ev("sample"),
        "whole_step": whole_step(cfg, B, T, st, headline_generate_ms if headline_generate_ms else full),
        "prefill": prefill_roofline(B, T, 300, cfg["num_heads"], d // cfg["num_heads"], f["semantic"].device),
        "forward": forward_leg(model, f, B, T, cfg),
    }


def whole_step(cfg, B, T, st, generate_ms):
    """SURVEY.md §8(d) step-level figure — the honest headline of the decode path: algorithmic bytes of one average decode step
    (decoder weights read once, the clips' cross-attention K/V, the self-attention K/V at the mean length) over the measured step time."""
    d, dff, nl, S = cfg["d_model"], cfg["dim_feedforward"], cfg["n_layers"], 300
    steps = T - 1
    weights = nl * (8 * d * d + 2 * d * dff) * 4 + (159 * d + (d + 1) * d) * 4
    kv = (st["self_attn_decode"]["bytes"] + st["cross_attn_decode"]["bytes"]) / steps
    us = 1e3 * generate_ms / steps
    return {"algorithmic_bytes_per_step": round(weights + kv), "us_per_step_incl_encode": round(us, 2),
            "achieved": round((weights + kv) / us / 1e3, 1), "unit": "GB/s", "frac": round((weights + kv) / us / 1e3 / HBM_PEAK_GBS, 4),
            "frac_of_achievable_6300": round((weights + kv) / us / 1e3 / 6300.0, 4),
            "note": "30 dependent launches per step inside a captured graph (the sampling head rides in the next step's first self-attention; "
                    "~1.2 us boundary each, profiles/r02_skinny_gemm_timeline_before.txt): the step is bound by the launch chain, the "
                    "streaming kernels by HBM"}


def v2_lockstep_leg(device, B=32, T=300, reps=3):
    """the reference's DEFAULT model family (`-music_gen_version 2.2`, utilities/argument_generate_funcs.py:82;
    model/video_music_transformer.py:316-609: rotary attention, three GLU layers + three SharedMoE(6 experts, top-2) layers) at the
    bench's width, decoded for B clips in lockstep to the reference's default length T = 300 (one captured step + decision graph,
    feedback-greedy).  Whole generate incl. video encode and cache initialisation; fp32."""
    from video2music_amd import _lib
    from video2music_amd.model.video_music_transformer import VideoMusicTransformer_V2
    cfg = dict(version_name="2.2", n_layers=6, num_heads=8, d_model=512, dim_feedforward=1024, max_sequence_chord=T,
               total_vf_dim=synthetic.total_vf_dim(1))
    m = VideoMusicTransformer_V2(**cfg).eval()
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=0).items()})
    m = m.to(device)
    f = {k: torch.from_numpy(v).to(device) for k, v in synthetic.synthetic_features(B, seed=5).items()}
    pr = [torch.tensor([v]) for v in C.primer_from_name("C")]

    def run(t):
        return m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], *pr, target_seq_length=t, beam=0,
                                sampler="argmax")

    with torch.no_grad():
        run(8)
        run(T)
        torch.cuda.synchronize(device)
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            out = run(T)
            torch.cuda.synchronize(device)
            best = min(best, time.perf_counter() - t0)
        short = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            run(T // 3)
            torch.cuda.synchronize(device)
            short = min(short, time.perf_counter() - t0)
    launches = int(_lib.call("amt_v2_last_step_launches"))
    return {"model": "VideoMusicTransformer_V2('2.2') 6+6 layers d_model=512 H=8 dff=1024, 6 experts top-2 + shared in layers 3-5",
            "batch": B, "seq_len": T, "tokens_per_s": round(B * (T - 1) / best, 1), "generate_ms": round(1e3 * best, 2),
            "launches_per_step": launches, "us_per_step_from_slope": round(1e6 * (best - short) / (T - T // 3), 2),
            "distinct_ids": len(set(out.flatten().tolist())), "dtype": "f32", "data": "synthetic",
            "measured": f"wall clock around generate_batch (encode + cache initialisation + {T - 1} replayed steps), best of {reps}; "
                        "the per-step figure is the slope between T and T/3"}


def rehearsal(args, rank, world):
    """AMT_BENCH_REHEARSAL=1 (tests/test_dist_gloo.py, no GPU): the launcher, the barriers, the one all_gather and the
    MAX-over-ranks reduction with fabricated ids in place of the generate.  The line says so and carries no rate."""
    B, T = args.batch, args.seq
    lo = rank * B
    toks = (torch.arange(lo, lo + B).view(-1, 1) * 10000 + torch.arange(T).view(1, -1)).long()
    torch.distributed.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = vdist.all_gather_sequences(toks, world * B)
    torch.distributed.barrier()
    te = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    torch.distributed.all_reduce(te, op=torch.distributed.ReduceOp.MAX)
    want = (torch.arange(world * B).view(-1, 1) * 10000 + torch.arange(T).view(1, -1)).long()
    assert torch.equal(out, want)
    if rank == 0:
        print(json.dumps({"metric": "rehearsal_only_no_generate", "value": None, "n_gpus": world, "steps": args.steps,
                          "data": "fabricated ids (AMT_BENCH_REHEARSAL=1)", "gathered": list(out.shape)}))
    torch.distributed.destroy_process_group()


def dump_outputs(path, ids, budget=64 << 20):
    """What the timed path hands its caller: the (clips, T) chord ids of the last step, as float32 (exact: ids < 2^24).  Above the
    budget, a fixed, seeded sample of whole clips."""
    ids = ids.cpu().numpy()
    cap = max(budget // (4 * ids.shape[1]), 1)
    if ids.shape[0] > cap:
        ids = ids[np.sort(np.random.RandomState(0).choice(ids.shape[0], cap, replace=False))]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "chord_ids.npy"), ids.astype(np.float32))


def main():
    args = parse_args()

    rank, world, local = vdist.init()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if os.environ.get("AMT_BENCH_REHEARSAL") == "1":
        return rehearsal(args, rank, world)
    device = torch.device("cuda", local % torch.cuda.device_count())    # ranks share a GPU only in gloo rehearsals
    torch.cuda.set_device(device)
    B, T = args.batch, args.seq
    heads = 8 if args.d_model >= 512 else 4
    cfg = dict(n_layers=args.layers, num_heads=heads, d_model=args.d_model, dim_feedforward=2 * args.d_model,
               max_sequence_chord=T, total_vf_dim=synthetic.total_vf_dim(1), rpr=True)
    model, sd = make_model(cfg, device)
    feats = synthetic.synthetic_features(B, seed=1234 + rank)
    f = {k: torch.from_numpy(v).to(device) for k, v in feats.items()}
    pr, prr, pra = (torch.tensor([v], device=device) for v in C.primer_from_name("C"))
    P = 1

    def step():
        toks = model.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra,
                                    target_seq_length=T, beam=0, sampler="argmax")
        return vdist.all_gather_sequences(toks, world * B)

    def barrier():
        torch.cuda.synchronize(device)
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(device)

    with torch.no_grad():
        if world > 1:
            # setup, not a step: the first collective creates the RCCL communicator (hundreds of ms) — keep it out of the timed
            # region even under --warmup 0
            vdist.all_gather_sequences(torch.zeros(B, T, dtype=torch.long, device=device), world * B)
        for _ in range(args.warmup):
            step()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = step()
        barrier()
        elapsed = time.perf_counter() - t0
    if world > 1:
        te = torch.tensor([elapsed], dtype=torch.float64, device=device if torch.distributed.get_backend() == "nccl" else "cpu")
        torch.distributed.all_reduce(te, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(te)
    assert out.shape == (world * B, T)
    tokens = world * B * (T - P) * args.steps
    result = {
        "metric": "chord_tokens_per_sec_generated", "value": round(tokens / elapsed, 1), "unit": "chord-tokens/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"AMT {args.layers}+{args.layers} layers d_model={args.d_model} H={heads} dff={2 * args.d_model} rpr, "
                               f"seq={T}, batch={B} clips/GPU x 300-frame video features (F={cfg['total_vf_dim']}), "
                               "feedback-greedy (G2) generate incl. video encode" + (" + all_gather of ids" if world > 1 else ""),
                   "global_batch": world * B, "seq_len": T, "parallelism": f"dp{world}"},
    }
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, out)
    full = args.full and rank == 0 and world == 1
    if full and not args.no_roofline:
        result["roofline"] = roofline(model, f, (pr, prr, pra), B, T, cfg, headline_generate_ms=1e3 * elapsed / args.steps)
        result["v2_lockstep"] = v2_lockstep_leg(device)
    if full and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(cfg, sd, T)
    if rank == 0:
        print(json.dumps(result))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
