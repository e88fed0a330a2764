"""profiles/reg_rest_train_step.json: one training step (forward, fused loss, backward, Adam) of the five regression heads that train
after `VideoRegression.enable_training()` -- 'mamba', 'mamba+', 'moemamba', 'cnngru', 'cnnbigru' -- at the regression CLI's defaults
(d_model 64, dim_feedforward 256, 2 layers, dropout 0.2) on 32 clips x 300 frames of 768 + 6 features (not a test; run on the GPU box).

    python tools/bench_reg_rest_train.py --remarks mamba.txt mamba_bwd.txt -o resources.json        # no GPU needed, see below
    python tools/bench_reg_rest_train.py --resources resources.json -o profiles/reg_rest_train_step.json

Per head: tools/bench_reg_train.py's method (device events around --steps steps after --warmup, best of --rounds, profiler off), then
the kernel breakdown of --trace-steps further steps under torch.profiler (device time per kernel name, launches per step).  For
'moemamba' also amt_selective_scan_wide_train_fwd beside amt_selective_scan_fwd at the head's own shape (B 32, L 300, ED 128, N 256):
the inference kernel is the instantiation the parent commit had (`selective_scan_wide_kernel<16, false>`, unchanged arithmetic), so
the difference is what the two extra stores (y_pre: B L ED floats; the checkpoints: B ceil(L / 32) ED N floats) cost.

--remarks: the compiler's resource-usage remarks for gfx950 of csrc/mamba.hip and csrc/mamba_bwd.hip,
`hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Rpass-analysis=kernel-resource-usage -c FILE -o /dev/null 2> FILE.txt`,
parsed into {kernel: {vgprs, sgprs, lds_bytes, scratch_bytes_per_lane, occupancy_waves_per_simd}} for the new kernels."""
import argparse
import collections
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEADS = ("mamba", "mamba+", "moemamba", "cnngru", "cnnbigru")
NEW_KERNELS = ("selective_scan_wide_kernelILi2ELb1", "selective_scan_wide_kernelILi4ELb1", "selective_scan_wide_kernelILi8ELb1",
               "selective_scan_wide_kernelILi16ELb1", "selective_scan_wide_bwd_kernel", "scan_wide_bwd_reduce_kernel", "silu_bwd_kernel")
FIELDS = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "LDS Size [bytes/block]": "lds_bytes", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
          "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}


def parse_remarks(paths):
    out, cur = {}, None
    for path in paths:
        for line in open(path):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = next((k for k in NEW_KERNELS if f"{len(k.split('IL')[0])}{k}" in m.group(1)), None)      # the mangled name: length, then name
                if cur:
                    out[cur] = {"symbol": m.group(1)}
                continue
            m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
            if m and cur and m.group(1) in FIELDS:
                out[cur][FIELDS[m.group(1)]] = int(m.group(2))
    missing = [k for k in NEW_KERNELS if k not in out]
    assert not missing, missing
    assert all(v["scratch_bytes_per_lane"] == 0 for v in out.values()), "a new kernel spills"
    return out


def timed(step, steps, warmup):
    import torch
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def breakdown(step, steps):
    """{kernel name: [device us per step, launches per step]}, largest first, under torch.profiler."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    acc = collections.defaultdict(lambda: [0.0, 0])
    for ev in prof.events():
        if ev.device_type is not None and "cuda" in str(ev.device_type).lower() and ev.device_time > 0:
            acc[ev.name][0] += ev.device_time
            acc[ev.name][1] += 1
    rows = sorted(((k, v[0] / steps, v[1] / steps) for k, v in acc.items()), key=lambda r: -r[1])
    total = sum(r[1] for r in rows)
    return {"device_us_per_step": total, "launches_per_step": sum(r[2] for r in rows),
            "kernels": [{"name": k[:120], "us_per_step": round(us, 2), "launches_per_step": n, "share": round(us / total, 4)} for k, us, n in rows[:24]]}


def scan_pair(a):
    import torch
    from video2music_amd import ops
    dev, B, L, ED, N, R = "cuda:0", a.batch, a.seq, 2 * a.d_model, 256, 4
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    M, ld = B * L, R + 2 * N
    xc, draw, dt_bias, dbc, D, xz = r(M, ED), 0.5 * r(M, ED), r(ED) - 1.0, 0.5 * r(M, ld), 1.0 + 0.1 * r(ED), r(M, 2 * ED)
    A_log = torch.log(torch.arange(1, N + 1, dtype=torch.float32, device=dev)).repeat(ED, 1).contiguous()
    args = (xc, draw, dt_bias, A_log, dbc, R, D, xz, B, L)
    fwd = min(timed(lambda: ops.selective_scan(*args, version=0), a.steps, a.warmup) for _ in range(a.rounds))
    trn = min(timed(lambda: ops.selective_scan_train(*args, version=0), a.steps, a.warmup) for _ in range(a.rounds))
    I = ops.scan_ckpt_steps(N)
    extra = 4 * (M * ED + B * -(-L // I) * ED * N)
    return {"shape": {"B": B, "L": L, "ED": ED, "N": N}, "amt_selective_scan_fwd_us": 1e3 * fwd, "amt_selective_scan_wide_train_fwd_us": 1e3 * trn,
            "extra_us": 1e3 * (trn - fwd), "extra_store_bytes": extra, "extra_bytes_at_6.3TBps_us": extra / 6.3e12 * 1e6,
            "note": "both figures include the Python wrapper's allocations (y; y_pre and the checkpoints for the training call)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--remarks", nargs="+")
    ap.add_argument("--resources")
    ap.add_argument("-o", "--out", required=True)
    ap.add_argument("--d_model", type=int, default=64)
    ap.add_argument("--d_hidden", type=int, default=256)
    ap.add_argument("--n_layers", type=int, default=2)
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=300)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-steps", type=int, default=3, help="0: no torch.profiler pass (a run under an external kernel trace)")
    ap.add_argument("--heads", default=",".join(HEADS), help="comma-separated subset; with one head and --trace-steps 0 the run suits "
                                                               "`rocprofv3 --kernel-trace --stats -- python tools/bench_reg_rest_train.py ...`")
    a = ap.parse_args()
    if a.remarks:
        json.dump(parse_remarks(a.remarks), open(a.out, "w"), indent=1)
        return
    import torch
    from video2music_amd import train_regression as TR
    from video2music_amd.losses import regression_train_loss
    from video2music_amd.model.video_regression import VideoRegression
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, S, F = a.batch, a.seq, 774
    sem, emo = torch.randn(B, S, F - 6, device=dev), torch.softmax(torch.randn(B, S, 6, device=dev), -1)
    nd, ld = 8 * torch.rand(B, S, device=dev), 4 * torch.rand(B, S, device=dev)
    inst = (torch.rand(B, S, 40, device=dev) < 0.25).float()
    res = {"config": {k: v for k, v in vars(a).items() if k not in ("remarks", "resources", "out")},
           "method": "device events around `steps` steps after `warmup`, best of `rounds`, profiler off; then the kernel breakdown of "
                     "`trace_steps` steps under torch.profiler (device time per kernel name, through roctracer).  profiles/reg_mamba_train_step.json's "
                     "breakdown came from a rocprofv3 kernel trace and tools/reg_train_breakdown.py instead; the two agree on what they "
                     "measure (a kernel's device time), the per-launch figures here carry the profiler's overhead on the host side only",
           "resource_usage_gfx950": json.load(open(a.resources)) if a.resources else None, "heads": {}}
    heads = [h for h in a.heads.split(",") if h]
    assert all(h in HEADS for h in heads), heads
    for rm in heads:
        m = VideoRegression(n_layers=a.n_layers, d_model=a.d_model, d_hidden=a.d_hidden, dropout=a.dropout, total_vf_dim=F, regModel=rm)
        m = m.to(dev).enable_training().train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-4, betas=(TR.ADAM_BETA_1, TR.ADAM_BETA_2), eps=TR.ADAM_EPSILON)

        def step():
            opt.zero_grad()
            ln_nd, p = m(sem, None, None, emo)
            regression_train_loss(ln_nd, p, nd, ld, inst).backward()
            opt.step()
        rounds = [timed(step, a.steps, a.warmup) for _ in range(a.rounds)]
        res["heads"][rm] = {"step_ms": min(rounds), "step_rounds_ms": rounds}
        try:
            if a.trace_steps > 0:
                res["heads"][rm]["breakdown"] = breakdown(step, a.trace_steps)
        except Exception as e:                                  # the profiler is not available: say so, keep the step time
            res["heads"][rm]["breakdown_error"] = f"{type(e).__name__}: {e}"[:300]
        print(rm, res["heads"][rm]["step_ms"], flush=True)
        json.dump(res, open(a.out, "w"), indent=1)
        del m, opt
    if a.trace_steps == 0:                                      # under an external trace: the steps alone
        return
    res["moemamba_scan_forward"] = scan_pair(a)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res["moemamba_scan_forward"]))


if __name__ == "__main__":
    main()
