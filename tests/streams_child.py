"""Three host threads, one probed stream each, in a process of their own (started once by tests/test_streams_gpu.py): the library's
one-time initialisations (its load, the big-LDS opt-in and the zero words of the decode GEMM, the autograd threads) happen for the
first time inside the race, which is why the threads run FIRST and the serial baseline -- the same jobs, one thread, the null stream --
afterwards.  Every round of every thread must equal that baseline bit for bit; the first difference ends the process with status 1
and is named.  Ten rounds check the contract; this is no stress loop, and an error in any thread stops all of them.

  thread 0  amt_decode_gemm_ex_fwd at B = 17 with its LayerNorm prologue (low product K1 = 256, N = 96; high product K = 512, N = 96),
            then amt_moe_fwd on the steered case 'full_plus_one' (a 128-row tile plus one row; the plan's integers are cleared per call)
  thread 1  LayerNormFn and RMSNormFn forward + backward at 129 rows x 512 with a residual, then chord_train_loss + backward at
            B = 2, L = 39 (the last-workgroup ticket on per-call workspaces)
  thread 2  AttentionFn forward + backward with relative positions and a keep mask, then selective_scan_train + selective_scan_bwd
            at reverse = 1"""
import ctypes
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import helpers_streams as HS  # noqa: E402

ROUNDS = 10
DEV = HS.DEV


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def jobs_thread0():
    from tests import helpers_ops_edges as H
    from video2music_amd import _lib
    B, K1, K2, n_low, n_high = 17, 256, 256, 96, 96
    K = K1 + K2
    rs = np.random.RandomState(11)
    rnd = lambda *s, scale=1.0: (rs.standard_normal(s) * scale).astype(np.float32)
    host = dict(x=rnd(B, K1), x2=rnd(B, K2) + 0.7, wl=rnd(n_low, K1, scale=K1 ** -0.5), bl=rnd(n_low, scale=0.1), wh=rnd(n_high, K, scale=K ** -0.5),
                bh=rnd(n_high, scale=0.1), fg=rnd(K1), fc=rnd(K1, scale=0.3), gam=1 + rnd(K2, scale=0.2), bet=rnd(K2, scale=0.1))
    c, inp = H.MOE_BY_NAME["full_plus_one"], H.moe_inputs("full_plus_one")
    assert c.k == 2 and not c.shared

    def gemm():
        D = {k: dev(v) for k, v in host.items()}
        yl, yh = torch.full((B, n_low), float("nan"), device=DEV), torch.full((B, n_high), float("nan"), device=DEV)
        sl, sh = torch.empty((n_low + 15) // 16 * 16 * K1, device=DEV), torch.empty((n_high + 15) // 16 * 16 * K, device=DEV)
        A = lambda k: _lib.addr(D[k])
        args = _lib.DecodeGemmArgs(x=A("x"), ldx=K1, x2=A("x2"), ldx2=K2, K1=K1, K=K, w_low=A("wl"), bias_low=A("bl"), resid=None, relu=0,
                                   w_high=A("wh"), bias_high=A("bh"), n_low=n_low, n_high=n_high, pro=1, fold_g=A("fg"), fold_c=A("fc"),
                                   ln_w=A("gam"), ln_b=A("bet"), y_low=_lib.addr(yl), y_high=_lib.addr(yh), scratch_low=_lib.addr(sl),
                                   scratch_high=_lib.addr(sh), B=B, eps=1e-5)
        _lib.call("amt_decode_gemm_ex_fwd", ctypes.byref(args), _lib.stream_ptr())
        return {"y_low": yl, "y_high": yh}

    def moe():
        P = _lib.ptr
        x, gw, gb = dev(inp["x"]), dev(inp["gate_w"]), dev(inp["gate_b"])
        ex = [dev(inp["experts"][k]) for k in ("w1", "b1", "wg", "bg", "w2", "b2")]
        n = _lib.call("amt_moe_scratch_floats", c.n_tok, c.d, c.dff, c.n_exp)
        scratch = torch.full((n,), float("nan"), device=DEV)
        out = torch.full((c.n_tok, c.d), float("nan"), device=DEV)
        idx = torch.full((c.n_tok, 2), -1, dtype=torch.int32, device=DEV)
        wts = torch.full((c.n_tok, 2), float("nan"), device=DEV)
        _lib.call("amt_moe_fwd", P(x), P(gw), P(gb), *[P(t) for t in ex], *([None] * 6), P(out), P(idx), P(wts), P(scratch), c.n_tok, c.d, c.dff,
                  c.n_exp, _lib.stream_ptr())
        return {"out": out, "idx": idx, "wts": wts}

    return [("decode_gemm B17 K512 N96 LayerNorm prologue", gemm), ("amt_moe_fwd full_plus_one", moe)]


def jobs_thread1():
    from tests import helpers_family_train as FT, test_chord_loss_gpu as CL, test_family_train_ops_gpu as FO, test_layernorm_bwd_gpu as LN
    from video2music_amd import losses
    rows, dim, resid = 129, 512, True
    ln, rms = LN.inputs(rows, dim, resid), FT.rms_inputs(rows, dim, resid)
    y, tgt, emo = CL.make_case(2, 39, 160)

    def chord():
        yd = dev(y, True)
        loss = losses.chord_train_loss(yd, torch.from_numpy(np.ascontiguousarray(tgt)), torch.from_numpy(np.ascontiguousarray(emo)), CL.LAM, 0.1)
        loss.backward()
        return {"loss": loss.detach(), "dlogits": yd.grad[..., :CL.NC]}

    return [("LayerNormFn 129x512 resid", lambda: LN.device(ln)), ("RMSNormFn 129x512 resid", lambda: FO.rms_device(rms)),
            ("chord_train_loss 2x39", chord)]


def jobs_thread2():
    from tests import test_attn_train_gpu as AT, test_mamba_bwd_gpu as MW
    from video2music_amd import ops
    case = (2, 2, 37, 37, 32, 1, 1, 37, 1, 1)                # relative positions, a keep mask
    assert case in AT.CASES
    a, keep = AT.make(*case)
    B, L, ED = 2, 33, 24
    c = MW.scan_case(B, L, ED, seed=B * 1000 + L)
    R, M, N = c["R"], B * L, MW.N

    def scan():
        d = {k: v.to(DEV) for k, v in c.items() if k != "R"}
        y, y_pre, h_chunks = ops.selective_scan_train(d["xc"], d["draw"], d["dt_bias"], d["A_log"], d["dbc"], R, d["D"], d["xz"], B, L, version=1,
                                                      reverse=1)
        dxz, ddbc = torch.zeros(M, 2 * ED, device=DEV), torch.zeros_like(d["dbc"])
        dx, ddraw, dA_log, dD = ops.selective_scan_bwd(d["dout"], d["xc"], d["draw"], d["dt_bias"], d["A_log"], d["dbc"], R, d["D"], d["xz"], y_pre,
                                                       h_chunks, dxz, ddbc, B, L, version=1, reverse=1)
        return {"y": y, "dx": dx, "ddraw": ddraw, "dz": dxz[:, ED:], "dBC": ddbc[:, R:R + 2 * N], "dA_log": dA_log, "dD": dD}

    return [("AttentionFn rpr keep-mask", lambda: AT.device(a, keep, case[1], case[5], case[8])), ("selective_scan reverse 1", scan)]


def main():
    e = HS.env()
    n_threads = min(3, len(e.streams))
    if n_threads < 3:                                        # fewer probed streams: the three job lists are dealt over the threads there are
        print(f"STREAMS_CHILD only {n_threads} independent streams: {n_threads} threads share the three job lists", flush=True)
    lists = [b() for b in (jobs_thread0, jobs_thread1, jobs_thread2)]       # host inputs only: no entry point has been called yet
    per_thread = [[j for k, jobs in enumerate(lists) if k % n_threads == t for j in jobs] for t in range(n_threads)]
    results = [[None] * ROUNDS for _ in range(n_threads)]
    errors, stop = [], threading.Event()
    barrier = threading.Barrier(n_threads)

    def work(t):
        try:
            torch.cuda.set_device(0)
            barrier.wait(60)
            with torch.cuda.stream(e.streams[t]):
                for r in range(ROUNDS):
                    if stop.is_set():
                        return
                    results[t][r] = {name: HS.flatten(fn()) for name, fn in per_thread[t]}
            e.streams[t].synchronize()
        except BaseException as exc:                         # noqa: BLE001 (a fault in one thread ends all of them)
            errors.append((t, repr(exc)))
            stop.set()
            barrier.abort()

    threads = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
    [t.start() for t in threads]
    [t.join(150) for t in threads]
    if errors or any(t.is_alive() for t in threads):
        print(f"STREAMS_CHILD failed: {errors or 'a thread did not finish'}", flush=True)
        os._exit(2)
    torch.cuda.synchronize()
    for t in range(n_threads):
        base = {name: HS.flatten(fn()) for name, fn in per_thread[t]}
        torch.cuda.synchronize()
        for name, b in base.items():
            HS.finite(b, name)
            for r in range(ROUNDS):
                try:
                    HS.same(results[t][r][name], b, f"thread {t} round {r}: {name} against the serial null-stream baseline")
                except AssertionError as exc:
                    print(f"STREAMS_CHILD differs: {exc}", flush=True)
                    sys.exit(1)
    HS.record(part=4, threads=n_threads, rounds=ROUNDS, jobs=[[n for n, _ in jobs] for jobs in per_thread], equal=True)
    print("STREAMS_CHILD ok", flush=True)


if __name__ == "__main__":
    main()
