"""Where a training step of a V1 / V2 chord model spends its device time, from a kernel trace of tools/bench_train.py:

    rocprofv3 --kernel-trace --stats -d OUT -o fam -- python tools/bench_train.py --music_gen_version 2.2 --skip_base --steps 5 --warmup 2 --rounds 1
    python tools/family_train_breakdown.py OUT/.../fam_results.db 7 > profiles/family_train_v22_kernels.json

Reads the trace's SQLite database (view `kernels`) and prints, per step, the twenty leading kernels and the share of the kernels of
csrc/family_train.hip and the RMSNorm backward of csrc/norm_bwd.hip; the second argument is the number of steps the traced run made (warm-up included).  The activation and
weight-gradient kernels are shared with the mixture layers (csrc/moe_train_kernels.h) and cannot be told apart by name: they are
reported together."""
import json
import sqlite3
import sys

NEW = (("rope_bwd_kernel", "rotary backward (rope_bwd_kernel)"), ("rope_kernel", "rotary forward (rope_kernel)"),
       ("norm_bwd_kernel<true>", "RMSNorm backward (norm_bwd_kernel<true>)"), ("norm_kernel<true>", "RMSNorm forward (norm_kernel<true>)"),
       ("moe_act_fwd_kernel", "GLU activation forward, plain layers and mixtures (moe_act_fwd_kernel)"),
       ("moe_bwd_act_kernel", "GLU activation backward, plain layers and mixtures (moe_bwd_act_kernel)"),
       ("moe_wgrad", "weight-gradient product, plain layers and mixtures (moe_wgrad_kernel / _reduce)"))


def main():
    db, steps = sys.argv[1], int(sys.argv[2])
    con = sqlite3.connect(db)
    rows = con.execute("select name, count(*), sum(end - start) from kernels group by name order by 3 desc").fetchall()
    total = sum(r[2] for r in rows)
    share = {}
    for key, label in NEW:
        sel = [r for r in rows if key in r[0]]
        share[label] = {"launches_per_step": round(sum(r[1] for r in sel) / steps, 1), "us_per_step": round(sum(r[2] for r in sel) / 1e3 / steps, 1),
                        "share": round(sum(r[2] for r in sel) / total, 4)}
    print(json.dumps({"steps_in_trace": steps, "device_ms_per_step": round(total / 1e6 / steps, 2),
                      "launches_per_step": round(sum(r[1] for r in rows) / steps, 1), "family_train_kernels": share,
                      "kernels": [{"name": r[0][:160], "calls_per_step": round(r[1] / steps, 1), "us_per_step": round(r[2] / 1e3 / steps, 1),
                                   "share": round(r[2] / total, 4)} for r in rows[:20]]}, indent=1))


if __name__ == "__main__":
    main()
