"""Where a regression-training step's device time goes, from a kernel trace of tools/bench_reg_train.py:

    rocprofv3 --kernel-trace --stats -d OUT -o reg_train -- python tools/bench_reg_train.py --which ours --steps 20 --warmup 3 --rounds 1
    python tools/reg_train_breakdown.py OUT/reg_train_results.db 23 profiles/reg_train_kernel_stats.csv > profiles/reg_train_breakdown.json

Reads the trace's SQLite database (view `kernels`), writes per-kernel totals as CSV and prints the per-step breakdown by kind as JSON;
the second argument is the number of steps the traced run made (warm-up included)."""
import csv
import json
import sqlite3
import sys

KINDS = (("moe_wgrad", "mixture layer: grouped weight-gradient product (moe_wgrad_kernel / _reduce)"),
         ("moe_bwd", "mixture layer: backward's row kernels (moe_bwd_dy / dlogit / act / dx)"),
         ("moe_", "mixture layer: router, plan, gating, combine"),
         ("selective_scan_wide_bwd", "wide scan backward (selective_scan_wide_bwd_kernel)"),
         ("scan_wide_bwd_reduce", "wide scan backward's ordered sums and element-wise part (scan_wide_bwd_reduce_kernel)"),
         ("selective_scan_wide_kernel", "wide scan forward (selective_scan_wide_kernel<NS, true>)"),
         ("selective_scan_bwd", "scan backward (selective_scan_bwd_kernel)"), ("scan_bwd_reduce", "scan backward's ordered sums (scan_bwd_reduce_kernel)"),
         ("selective_scan_kernel", "scan forward (selective_scan_kernel<16, true>)"), ("dwconv_silu_bwd", "conv backward (dwconv_silu_bwd / _reduce)"),
         ("dwconv_silu_dacc", "conv backward (dwconv_silu_dacc_kernel)"), ("dwconv_silu", "conv forward (dwconv_silu_kernel)"),
         ("silu_bwd_kernel", "dense conv front's SiLU derivative (silu_bwd_kernel)"), ("norm_bwd_kernel<true>", "RMSNorm backward"),
         ("norm_bwd_kernel<false>", "LayerNorm backward"), ("norm_kernel", "LayerNorm forward"),
         ("rnn_seq_bwd", "recurrence backward (rnn_seq_bwd_kernel)"), ("rnn_seq_train", "recurrence forward (rnn_seq_train_kernel)"),
         ("reg_loss", "fused loss (reg_loss_kernel)"), ("gemm_f32_kernel", "dense GEMM (gemm_f32_kernel)"), ("decode_gemm", "skinny GEMM"),
         ("concat2", "concat2"), ("direct_copy", "torch copies (transposed / padded operands, h_prev, slices)"),
         ("FillFunctor", "torch fills (zeros of the padded copies, zero_grad)"), ("multi_tensor", "Adam (torch multi-tensor kernels)"),
         ("fillBuffer", "memset (loss ticket)"))
OTHER = "other torch elementwise (dropout masks and multiplies, cat, gradient scaling)"


def kind(name):
    return next((label for key, label in KINDS if key in name), OTHER)


def main():
    db, steps, out_csv = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    con = sqlite3.connect(db)
    rows = con.execute("select name, count(*), sum(end - start), avg(end - start), min(end - start), max(end - start) from kernels "
                       "group by name order by 3 desc").fetchall()
    total = sum(r[2] for r in rows)
    with open(out_csv, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs"])
        for r in rows:
            w.writerow([r[0], r[1], r[2], round(r[3], 1), round(100 * r[2] / total, 2), r[4], r[5]])
    kinds = {}
    for name, calls, ns, *_ in rows:
        k = kinds.setdefault(kind(name), [0, 0])
        k[0] += calls
        k[1] += ns
    by_grid = con.execute("select grid_x / workgroup_x, count(*), avg(end - start) from kernels where name like '%gemm_f32_kernel%' "
                          "group by grid_x order by 3 desc").fetchall()
    print(json.dumps({"steps": steps, "device_us_per_step": round(total / 1e3 / steps, 1), "launches_per_step": round(sum(r[1] for r in rows) / steps, 1),
                      "by_kind": {label: {"launches_per_step": round(v[0] / steps, 1), "us_per_step": round(v[1] / 1e3 / steps, 1),
                                          "share": round(v[1] / total, 3)} for label, v in sorted(kinds.items(), key=lambda kv: -kv[1][1])},
                      "dense_gemm_by_workgroups": [{"workgroups": int(g), "launches": n, "avg_us": round(a / 1e3, 1)} for g, n, a in by_grid]}, indent=1))


if __name__ == "__main__":
    main()
