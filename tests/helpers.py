"""Shared helpers for the parity tests (test infrastructure)."""
import numpy as np
import torch

from video2music_amd import synthetic

CFG1 = dict(n_layers=2, num_heads=4, d_model=128, dim_feedforward=256, max_sequence_chord=300,
            total_vf_dim=synthetic.total_vf_dim(1), rpr=True)
CFG2 = dict(n_layers=6, num_heads=8, d_model=512, dim_feedforward=1024, max_sequence_chord=1024,
            total_vf_dim=synthetic.total_vf_dim(1), rpr=True)


def amt_named_shapes(n_layers, num_heads, d_model, dim_feedforward, max_sequence_chord, total_vf_dim, **_):
    """(name, shape) list of the reference VideoMusicTransformer state_dict."""
    d, ff, F = d_model, dim_feedforward, total_vf_dim
    hd = d // num_heads
    out = [("embedding.weight", (159, d)), ("embedding_root.weight", (15, d)), ("embedding_attr.weight", (16, d)),
           ("Linear_vis.weight", (d, F)), ("Linear_vis.bias", (d,)),
           ("Linear_chord.weight", (d, d + 1)), ("Linear_chord.bias", (d,)),
           ("condition_linear.weight", (d, 1)), ("condition_linear.bias", (d,))]

    def attn(p, er):
        o = [(p + "in_proj_weight", (3 * d, d)), (p + "in_proj_bias", (3 * d,))]
        if er:
            o.append((p + "Er", (max_sequence_chord, hd)))
        return o + [(p + "out_proj.weight", (d, d)), (p + "out_proj.bias", (d,))]

    def ffn(p, nn):
        o = [(p + "linear1.weight", (ff, d)), (p + "linear1.bias", (ff,)),
             (p + "linear2.weight", (d, ff)), (p + "linear2.bias", (d,))]
        for i in range(1, nn + 1):
            o += [(p + f"norm{i}.weight", (d,)), (p + f"norm{i}.bias", (d,))]
        return o

    for i in range(n_layers):
        p = f"transformer.encoder.layers.{i}."
        out += attn(p + "self_attn.", False) + ffn(p, 2)
    out += [("transformer.encoder.norm.weight", (d,)), ("transformer.encoder.norm.bias", (d,))]
    for i in range(n_layers):
        p = f"transformer.decoder.layers.{i}."
        out += attn(p + "self_attn.", True) + attn(p + "multihead_attn.", False) + ffn(p, 3)
    out += [("transformer.decoder.norm.weight", (d,)), ("transformer.decoder.norm.bias", (d,)),
            ("Wout_root.weight", (15, d)), ("Wout_root.bias", (15,)),
            ("Wout_attr.weight", (16, d)), ("Wout_attr.bias", (16,)),
            ("Wout.weight", (159, d)), ("Wout.bias", (159,))]
    return out


def synthetic_sd(cfg, seed=0, dtype=torch.float32, recipe="default"):
    sd = synthetic.synthetic_state_dict(amt_named_shapes(**cfg), seed=seed, recipe=recipe)
    return {k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}


def feats_t(feats, sl=slice(None), key=None, dtype=torch.float32):
    f = {k: torch.from_numpy(np.ascontiguousarray(v[sl])).to(dtype) for k, v in feats.items()}
    if key is not None:
        f["key"] = torch.from_numpy(np.ascontiguousarray(key[sl])).to(dtype)
    return f


CFG_V2 = dict(version_name="2.2", n_layers=6, num_heads=4, d_model=128, dim_feedforward=256, max_sequence_chord=300,
              total_vf_dim=synthetic.total_vf_dim(1))


def v2_named_shapes(n_layers, num_heads, d_model, dim_feedforward, total_vf_dim, n_experts=6, **_):
    """(name, shape) list of the reference VideoMusicTransformer_V2('2.2') state_dict."""
    d, ff, F = d_model, dim_feedforward, total_vf_dim
    out = [("embedding.weight", (159, d)), ("embedding_root.weight", (15, d)), ("embedding_attr.weight", (16, d)),
           ("Linear_vis.weight", (d, F)), ("Linear_vis.bias", (d,)),
           ("Linear_chord.weight", (d, d + 1)), ("Linear_chord.bias", (d,)),
           ("condition_linear.weight", (d, 1)), ("condition_linear.bias", (d,))]

    def attn(p):
        return [(p + "in_proj_weight", (3 * d, d)), (p + "in_proj_bias", (3 * d,)), (p + "out_proj.weight", (d, d)), (p + "out_proj.bias", (d,))]

    def glu(p):
        return [(p + "linear1.weight", (ff, d)), (p + "linear1.bias", (ff,)), (p + "linear2.weight", (d, ff)), (p + "linear2.bias", (d,)),
                (p + "gate.weight", (ff, d)), (p + "gate.bias", (ff,))]

    def ffn(p, deep):
        if not deep:
            return glu(p)
        o = []
        for e in range(n_experts):
            o += glu(p + f"experts.{e}.")
        return o + [(p + "gate.weight", (n_experts, d)), (p + "gate.bias", (n_experts,))] + glu(p + "shared_expert.")

    def norms(p, n):
        o = []
        for i in range(1, n + 1):
            o += [(p + f"norm{i}.weight", (d,)), (p + f"norm{i}.bias", (d,))]
        return o

    for stack, nn_ in (("encoder", 2), ("decoder", 3)):
        for i in range(n_layers):
            p = f"transformer.{stack}.layers.{i}."
            out += attn(p + "self_attn.")
            if stack == "decoder":
                out += attn(p + "cross_attn.")
            out += ffn(p + "ff.", i >= 3) + norms(p, nn_)
        out += [(f"transformer.{stack}.norm.weight", (d,)), (f"transformer.{stack}.norm.bias", (d,))]
    return out + [("Wout.weight", (159, d)), ("Wout.bias", (159,))]


def synthetic_sd_v2(cfg, seed=0, recipe="default"):
    sd = synthetic.synthetic_state_dict(v2_named_shapes(**cfg), seed=seed, recipe=recipe)
    return {k: torch.from_numpy(v) for k, v in sd.items()}


# ---- the lockstep V1 / V2 step, teacher-forced (tests/test_lockstep_parity_gpu.py) ----------------------------------------------
def lockstep_step_logits(m, f, roots, attrs):
    """Logits (T, B, 159) of the lockstep step (amt_v2_step_batch) teacher-forced along per-clip (root, attr) ids (B, T) -- chord
    ids in `roots` for chord_embed -- driven like the host-decision branch of `generate_batch`: `state[1:]` = this position's
    (root, attr) of every clip, the step advances the position.  `f`: B clips of features on the device."""
    B, T = roots.shape
    dev = m.Wout.weight.device
    with torch.no_grad():
        rows, _, S = m._encode_memory(f["semantic"], f["scene_offset"], f["motion"], f["emotion"], clips=True)
        st = m._cache_init([rows[c * S:(c + 1) * S] for c in range(B)], S)
        assert st["native"], "the configuration does not take the lockstep step"
        keys = f["key"].to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        state = torch.zeros(1 + 2 * B, dtype=torch.int32, device=dev)
        out = torch.empty(T, B, 159, device=dev)
        for t in range(T):
            state[1:] = torch.cat((roots[:, t], attrs[:, t])).to(device=dev, dtype=torch.int32)
            m._step_batch(st, keys, state)
            out[t] = st["logits"].view(B, 159)
        assert int(state[0]) == T
    return out.cpu()


def one_clip_step_logits(m, f, roots, attrs):
    """Logits (T, 159) of the one-clip step (amt_v2_step, what per-clip `generate` takes with decision="host") teacher-forced
    along (root, attr) ids (T,) of clip 0 of `f`."""
    T = roots.shape[0]
    with torch.no_grad():
        memory, B, S = m._encode_memory(f["semantic"][:1], f["scene_offset"][:1], f["motion"][:1], f["emotion"][:1])
        st = m._cache_init(memory, S)
        assert st["native"], "the configuration does not take the one-call step"
        key = float(f["key"].reshape(-1)[0])
        out = torch.stack([m._decode_step_native(int(roots[t]), int(attrs[t]), key, t, st).clone() for t in range(T)])
    return out.cpu()


def decision_inputs(toks, P, primer_root, primer_attr, beam, chord_embed):
    """(root, attr) ids (B, T) the lockstep decision fed back along generated ids `toks` (B, T) -- `_lockstep_loop`: the primer's,
    then chord_to_root_attr of each id (beam 0), the pad ids (top-1, no feedback), or the id itself with attr 0 (chord_embed)."""
    from video2music_amd.utilities.constants import CHORD_ATTR_PAD, CHORD_ROOT_PAD, chord_to_root_attr
    toks = toks.cpu()
    B, T = toks.shape
    roots = torch.full((B, T), CHORD_ROOT_PAD, dtype=torch.long)
    attrs = torch.full((B, T), CHORD_ATTR_PAD, dtype=torch.long)
    if chord_embed:
        return toks.clone(), torch.zeros(B, T, dtype=torch.long)
    roots[:, :P], attrs[:, :P] = primer_root, primer_attr
    if beam == 0:
        for b in range(B):
            for t in range(P, T):
                roots[b, t], attrs[b, t] = chord_to_root_attr(int(toks[b, t]))
    return roots, attrs


def _decision_probs(lg, toks, b, cur, max_conseq_N, max_conseq_chord, temperature, suppress=True):
    from video2music_amd.utilities.constants import CHORD_END
    pr = torch.softmax(lg / temperature, -1)[:CHORD_END].numpy().copy()
    if suppress:
        if max_conseq_N == 0:
            pr[0] = 0.0
        if cur >= max_conseq_chord and all(toks[b, cur - 1] == toks[b, cur - 1 - k] for k in range(1, max_conseq_chord)):
            pr[toks[b, cur - 1]] = 0.0
    return pr


def check_draws(toks, logits, u, P, max_conseq_N, max_conseq_chord, temperature=1.0):
    """Every generated id is the inverse-CDF draw of the reference's decision distribution (:1085-1105) at its uniform:
    recomputed in fp64 from the returned logits, with a band for fp32 rounding of the device's cumulative sums."""
    toks, logits, u = toks.cpu().numpy(), logits.cpu().double(), u.cpu().double().numpy()
    B, T = toks.shape
    for b in range(B):
        for cur in range(P, T):
            pr = _decision_probs(logits[cur - 1, b], toks, b, cur, max_conseq_N, max_conseq_chord, temperature)
            cdf = np.cumsum(pr)
            tok, target = int(toks[b, cur]), u[cur - 1, b] * cdf[-1]
            assert pr[tok] > 0.0, (b, cur, tok)
            assert (cdf[tok] - pr[tok]) - 1e-5 <= target <= cdf[tok] + 1e-5, (b, cur, tok, target, cdf[tok] - pr[tok], cdf[tok])


def check_argmax(toks, logits, P, max_conseq_N, max_conseq_chord, temperature=1.0, beam=0):
    """Every generated id is the arg-max of the decision distribution (beam 0 with sampler="argmax": after the N / repeat
    suppression; beam 1, top-1: none), recomputed in fp64 from the logits, or within 1e-6 of it (a tie at fp32 rounding)."""
    toks, logits = toks.cpu().numpy(), logits.cpu().double()
    B, T = toks.shape
    for b in range(B):
        for cur in range(P, T):
            pr = _decision_probs(logits[cur - 1, b], toks, b, cur, max_conseq_N, max_conseq_chord, temperature, suppress=beam == 0)
            pr /= pr.sum()
            tok = int(toks[b, cur])
            assert pr[tok] > 0.0 and pr[tok] >= pr.max() - 1e-6, (b, cur, tok, pr[tok], int(pr.argmax()), pr.max())


def boundary_uniforms(toks, logits, P, max_conseq_N, max_conseq_chord, temperature=1.0, margin=2e-5):
    """Uniforms (T, B) that put each draw of `toks` `margin` (of the total mass) inside its inverse-CDF interval, at the lower edge
    for even positions and the upper edge for odd ones (the middle of an interval narrower than 2 margin): a decision whose CDF is
    off by more than `margin` at some boundary moves an id, while the exact one repeats `toks`."""
    toks, logits = toks.cpu().numpy(), logits.cpu().double()
    B, T = toks.shape
    u = np.full((T, B), 0.5)
    for b in range(B):
        for cur in range(P, T):
            pr = _decision_probs(logits[cur - 1, b], toks, b, cur, max_conseq_N, max_conseq_chord, temperature)
            pr /= pr.sum()
            tok = int(toks[b, cur])
            lo = pr[:tok].sum()
            if pr[tok] < 2 * margin:
                u[cur - 1, b] = lo + pr[tok] / 2
            else:
                u[cur - 1, b] = lo + margin if cur % 2 == 0 else lo + pr[tok] - margin
    return torch.from_numpy(u.astype(np.float32))
