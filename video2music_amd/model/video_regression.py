"""`VideoRegression` (reference model/video_regression.py:104-245) for the Mamba regModels: 'bimamba+' -- the default
regression head of both callers (utilities/argument_generate_funcs.py:87-91, video2music.py:651) --, 'bimamba' (the same
encoder over the original Mamba gate), and the one-directional stacks 'mamba' / 'mamba+' (mamba.py:66-100,131-147:
x + MambaBlock(RMSNorm(x)) per layer), 'moe_bimamba+' / 'sharedmoe_bimamba+' (a mixture layer in the FFN's place), and the
recurrent heads 'lstm' / 'bilstm' / 'gru' / 'bigru' / 'cnngru' / 'cnnbigru' (torch's nn.LSTM / nn.GRU, kept as parameter
containers; the recurrence runs in csrc/rnn.hip).  Per video frame it predicts (note density, loudness) and 40 instrument
probabilities from cat(semantic, emotion) — SURVEY.md §8 row f2.

The module keeps the reference's parameter names (so `load_state_dict(torch.load(path))` works) and composes the
library's kernels; no torch arithmetic runs in `forward`:

    cat + zero-pad            amt_concat2_fwd
    every nn.Linear           amt_linear_ex_fwd (bias / residual / ReLU / sigmoid in the GEMM epilogue)
    Conv1d + SiLU             amt_dwconv1d_silu_fwd
    softplus, scan, gate      amt_selective_scan_fwd
    LayerNorms                amt_layernorm_post_fwd (residual in, `x_f + x_b` out)
    LSTM / GRU recurrence     amt_rnn_seq_fwd (both directions of a layer in one launch); d_model above 128, accepted with
                              `wide_recurrent=True` (multiples of 32 up to 512): amt_rnn_wide_seq_fwd, one launch per time step

The backward Mamba block runs with `reverse=1` instead of `torch.flip` before and after (bimamba.py:171-185).

Training: for 'lstm' / 'bilstm' / 'gru' / 'bigru' and for 'bimamba+' / 'bimamba', `forward` / `get_feature` called in the training
state with gradients enabled build their result through the autograd Functions of `video2music_amd/autograd.py` on the module's own
parameters (amt_rnn_seq_train_fwd / amt_rnn_seq_bwd; amt_selective_scan_train_fwd / amt_selective_scan_bwd / amt_dwconv1d_silu_bwd /
amt_layernorm_bwd; the same GEMMs), so `loss.backward()` and a torch optimiser work; every other state and regModel runs the
inference path above on detached parameters.  'moe_bimamba+' / 'sharedmoe_bimamba+' train too: their mixture layer goes through
autograd.MoEFn (amt_moe_train_fwd / amt_moe_bwd).

The other five heads train after `enable_training()` (an opt-in: a module that never called it runs the inference path in every
state, as before): 'mamba' / 'mamba+' through autograd.RMSNormFn (amt_rmsnorm_bwd) around MambaBlockFn; 'moemamba' the same with
its blocks' d_state = d_hidden states per channel on the wide-state training scan (amt_selective_scan_wide_train_fwd /
amt_selective_scan_wide_bwd) and its mixture layer through MoEFn; 'cnngru' / 'cnnbigru' through autograd.ConvSiluFn (the seven GEMMs
of the convolution front, amt_silu_bwd) in front of RnnLayerFn.
"""
import math

import torch
import torch.nn as nn

from .. import ops
from .._derived import HasDerived

INSTRUMENT_SIZE = 40            # utilities/constants.py:84


class _MambaBlockParams(nn.Module):
    """Parameters of MambaBlock (mamba.py:160-231) with bias=True, conv_bias=True, no inner layernorms."""

    def __init__(self, d_model, d_state=16, expand=2, d_conv=4):
        super().__init__()
        self.d_inner, self.d_state, self.d_conv = expand * d_model, d_state, d_conv
        self.dt_rank = math.ceil(d_model / 16)
        self.in_proj = nn.Linear(d_model, 2 * self.d_inner)
        self.conv1d = nn.Conv1d(self.d_inner, self.d_inner, d_conv, groups=self.d_inner, padding=d_conv - 1)
        self.x_proj = nn.Linear(self.d_inner, self.dt_rank + 2 * d_state, bias=False)
        self.dt_proj = nn.Linear(self.dt_rank, self.d_inner)
        self.A_log = nn.Parameter(torch.log(torch.arange(1, d_state + 1, dtype=torch.float32).repeat(self.d_inner, 1)))
        self.D = nn.Parameter(torch.ones(self.d_inner))
        self.out_proj = nn.Linear(self.d_inner, d_model)


class _BiMambaLayerParams(nn.Module):
    """BiMambaEncoderLayer_V1 (bimamba.py:102-133): plain FFN, or a copy of `moe` (a mixture layer) in its place."""

    def __init__(self, d_model, d_hidden, moe=None):
        super().__init__()
        self.mamba_forward = _MambaBlockParams(d_model)
        self.mamba_backward = _MambaBlockParams(d_model)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(d_model), nn.LayerNorm(d_model), nn.LayerNorm(d_model)
        if moe is None:
            self.ffn = nn.Sequential(nn.Linear(d_model, d_hidden), nn.ReLU(), nn.Dropout(0.0), nn.Linear(d_hidden, d_model))
        else:
            import copy
            self.ffn = copy.deepcopy(moe)


class _RMSWeight(nn.Module):
    """mamba.py's RMSNorm (:472-489): a gain vector, eps 1e-5."""

    def __init__(self, d_model, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(d_model))


class _ResidualBlockParams(nn.Module):
    """ResidualBlock (mamba.py:131-147): keys mixer.*, norm.weight."""

    def __init__(self, d_model, d_state=16, d_conv=4):
        super().__init__()
        self.mixer = _MambaBlockParams(d_model, d_state=d_state, d_conv=d_conv)
        self.norm = _RMSWeight(d_model)


class _ResidualMoEParams(nn.Module):
    """ResidualMoE (mamba.py:117-129): keys moe_layer.*, norm.weight."""

    def __init__(self, moe, d_model):
        super().__init__()
        import copy
        self.moe_layer = copy.deepcopy(moe)
        self.norm = _RMSWeight(d_model)


class _MoEMambaParams(nn.Module):
    """MoEMamba (mamba.py:102-115): layers.{i}.0 = ResidualBlock, layers.{i}.1 = ResidualMoE."""

    def __init__(self, moe, d_model, d_state, d_conv, n_layers):
        super().__init__()
        self.layers = nn.ModuleList([nn.Sequential(_ResidualBlockParams(d_model, d_state, d_conv), _ResidualMoEParams(moe, d_model))
                                     for _ in range(n_layers)])


class _MambaStackParams(nn.Module):
    def __init__(self, d_model, n_layers):
        super().__init__()
        self.layers = nn.ModuleList([_ResidualBlockParams(d_model) for _ in range(n_layers)])


class _BiMambaLayerV0Params(nn.Module):
    """BiMambaEncoderLayer (bimamba.py:33-59), the layer of use_version 0 ('bimamba'): one FFN + norm pair per direction."""

    def __init__(self, d_model, d_hidden):
        super().__init__()
        self.mamba_forward = _MambaBlockParams(d_model)
        self.mamba_backward = _MambaBlockParams(d_model)
        self.norm1, self.norm2, self.norm3, self.norm4 = (nn.LayerNorm(d_model) for _ in range(4))
        self.ffn1 = nn.Sequential(nn.Linear(d_model, d_hidden), nn.ReLU(), nn.Dropout(0.0), nn.Linear(d_hidden, d_model))
        self.ffn2 = nn.Sequential(nn.Linear(d_model, d_hidden), nn.ReLU(), nn.Dropout(0.0), nn.Linear(d_hidden, d_model))


class _BiMambaEncoderParams(nn.Module):
    def __init__(self, d_model, d_hidden, n_layers, version=1, moe=None):
        super().__init__()
        if version == 1:                                                                # bimamba.py:16-19
            self.layers = nn.ModuleList([_BiMambaLayerParams(d_model, d_hidden, moe) for _ in range(n_layers)])
        else:
            self.layers = nn.ModuleList([_BiMambaLayerV0Params(d_model, d_hidden) for _ in range(n_layers)])


class VideoRegression(HasDerived, nn.Module):
    def __init__(self, n_layers=2, d_model=64, d_hidden=1024, dropout=0.1, use_KAN=False, max_sequence_video=300,
                 total_vf_dim=0, regModel="bilstm", scene_embed=False, chord_embed=False, *, wide_recurrent=False):
        super().__init__()
        if regModel not in ("bimamba+", "bimamba", "mamba", "mamba+", "moe_bimamba+", "sharedmoe_bimamba+", "lstm", "bilstm", "gru", "bigru",
                            "cnngru", "cnnbigru", "moemamba"):
            raise NotImplementedError("built: every regModel of video_regression.py:124-178 ('bimamba+' is the callers' default); 'minGRU' has "
                                      "no branch there either")
        self._version = 1 if regModel.endswith("+") else 0           # MambaConfig.use_version: 1 = the Mamba+ gate
        self._bidirectional = "bimamba" in regModel
        moe = None
        if regModel in ("moe_bimamba+", "sharedmoe_bimamba+", "moemamba"):     # GLUExpert(d, 2d + 1), 6 experts, top-2 (:143-178)
            from .moe import GLUExpert, MoELayer, SharedMoELayer
            cls = MoELayer if regModel == "moe_bimamba+" else SharedMoELayer
            moe = cls(GLUExpert(d_model, d_model * 2 + 1), d_model, n_experts=6, n_experts_per_token=2, dropout=dropout)
        if use_KAN or scene_embed or chord_embed:
            raise NotImplementedError("use_KAN / scene_embed / chord_embed are outside this path")
        recurrent = regModel in ("lstm", "bilstm", "gru", "bigru", "cnngru", "cnnbigru")
        if wide_recurrent and recurrent and d_model > ops.RNN_NARROW_MAX and (d_model % 32 != 0 or d_model > 512):
            raise ValueError("wide_recurrent: above 128 the recurrent heads stream W_hh onto the matrix pipe (csrc/rnn_wide.hip): d_model must be "
                             f"a multiple of 32, at most 512 (got {d_model})")
        if d_model % 32 != 0 or (d_hidden % 32 != 0 and regModel != "moemamba"):       # 'moemamba': d_hidden is d_state, no GEMM's K
            raise ValueError("d_model and d_hidden must be multiples of 32 (GEMM K step)")
        if d_model > 512 and regModel not in ("lstm", "bilstm", "gru", "bigru", "cnngru", "cnnbigru"):
            raise ValueError("the Mamba regModels take d_model <= 512: dt_rank = ceil(d_model / 16) must fit the 32 columns of `dbc` that the "
                             "dt projection reads")
        self.n_layers, self.d_model, self.d_hidden = n_layers, d_model, d_hidden
        self.max_seq_video, self.total_vf_dim, self.regModel = max_sequence_video, total_vf_dim, regModel
        self._rnn = recurrent
        if self._rnn:
            # torch's own modules as parameter containers (same keys: weight_ih_l0, ..., *_reverse); their forward is never called
            if (d_model > 128 and not wide_recurrent) or d_model % 8:
                raise ValueError("the recurrent heads keep W_hh in registers: d_model must be a multiple of 8, at most 128")
            cls = nn.LSTM if "lstm" in regModel else nn.GRU
            self._dirs = 2 if "bi" in regModel else 1
            rnn = cls(d_model, d_model, n_layers, bidirectional=self._dirs == 2, dropout=dropout, batch_first=True)
            if regModel.startswith("cnn"):                # CNN_GRU (:84-103): Conv1d(k=7, pad=3) + SiLU, then the GRU
                self.model = nn.Module()
                self.model.cnn = nn.Sequential(nn.Conv1d(d_model, d_model, kernel_size=7, stride=1, padding=3), nn.SiLU(), nn.Dropout(dropout))
                self.model.gru = rnn
            else:
                self.model = rnn
            self.__dict__["_rnn_mod"] = rnn          # an alias outside the module registry (no second set of keys)
        elif regModel == "moemamba":                      # MoEMamba over blocks with d_state = d_hidden, d_conv = 8 (:143-150)
            if d_hidden not in (16, 32, 64, 128, 256):
                raise ValueError("'moemamba' uses d_state = d_hidden: the scan kernel takes 16, 32, 64, 128 or 256 states per channel")
            self.model = _MoEMambaParams(moe, d_model, d_hidden, 8, n_layers)
        else:
            self.model = (_BiMambaEncoderParams(d_model, d_hidden, n_layers, self._version, moe) if self._bidirectional
                          else _MambaStackParams(d_model, n_layers))
        self.in_proj = nn.Sequential(nn.Linear(total_vf_dim, d_model), nn.Dropout(dropout))
        width = d_model * (self._dirs if self._rnn else 1)           # bidirectional recurrent heads: 2 d_model (:201-206)
        self.regressor = nn.Linear(width, 2)
        self.classifier = nn.Sequential(nn.Linear(width, INSTRUMENT_SIZE), nn.Sigmoid())
        self.dropout_masks = None       # training state: multipliers to use in place of drawn ones (see _get_feature_train)
        self._training_enabled = False  # enable_training(): the opt-in of the heads in OPT_IN_TRAINABLE

    OPT_IN_TRAINABLE = ("mamba", "mamba+", "moemamba", "cnngru", "cnnbigru")

    def enable_training(self):
        """Lets 'mamba' / 'mamba+' / 'moemamba' / 'cnngru' / 'cnnbigru' build an autograd graph in the training state with gradients
        enabled (the other heads do without being asked).  Eval mode and no_grad run what they ran before.  Returns self."""
        self._training_enabled = True
        return self

    def _derived(self):
        """-> (Fpad, Win, Wdt, Wx): zero-padded copies of the weights whose K (or row count) does not fit the GEMM's steps (rebuilt when
        they change): the padded feature width, the in-projection padded to it, per Mamba block the padded dt and x projections."""
        if self._rnn:                                   # only the in-projection needs a padded copy
            ws, xs = [self.in_proj[0].weight], []
        else:
            blocks = ([m for l in self.model.layers for m in (l.mamba_forward, l.mamba_backward)] if self._bidirectional
                      else [(l[0] if isinstance(l, nn.Sequential) else l).mixer for l in self.model.layers])
            ws = [self.in_proj[0].weight] + [m.dt_proj.weight for m in blocks]
            xs = [m.x_proj.weight for m in blocks]

        def build():
            dev = ws[0].device
            F = self.total_vf_dim
            Fpad = (F + 31) // 32 * 32
            Win = torch.zeros(self.d_model, Fpad, device=dev)
            Win[:, :F] = ws[0].detach()
            Wdt, Wx = [], []
            for w in ws[1:]:                       # (d_inner, dt_rank) -> (d_inner, 32): the GEMM reads dt | B | C[:..] x zeros
                t = torch.zeros(w.shape[0], 32, device=dev)
                t[:, :w.shape[1]] = w.detach()
                Wdt.append(t)
            for w in xs:                           # (dt_rank + 2N, d_inner): rows padded to a multiple of 4 (row stride of dbc)
                t = torch.zeros((w.shape[0] + 3) // 4 * 4, w.shape[1], device=dev)
                t[:w.shape[0]] = w.detach()
                Wx.append(t)
            return Fpad, Win, Wdt, Wx

        return self._tables.get("derived", ws + xs, build, wait=not self.training or not self._train_path())

    def packed_heads(self):
        """Both heads as the one packed, transposed tensor `ops.reg_metrics` reads (`ops.pack_reg_heads`); rebuilt when a head
        parameter changes."""
        ps = (self.regressor.weight, self.regressor.bias, self.classifier[0].weight, self.classifier[0].bias)
        return self._tables.get("heads", ps, lambda: ops.pack_reg_heads(*ps))

    def _conv7_silu(self, x, B, S):
        """CNN_GRU's Conv1d(d, d, kernel 7, padding 3) + SiLU over time (:88-91, :97-100) as seven accumulating GEMMs: the clips
        are laid end to end with 3 zero frames on each side, tap j of output row r reads row r + j; the SiLU rides on the last one."""
        conv = self.model.cnn[0]
        d, K = self.d_model, conv.kernel_size[0]
        pad = K // 2
        W = conv.weight.detach()                                   # (d_out, d_in, K)
        xp = torch.zeros(B, S + 2 * pad, d, device=x.device, dtype=torch.float32)
        xp[:, pad:pad + S] = x.view(B, S, d)
        flat = xp.view(B * (S + 2 * pad), d)
        M = flat.shape[0] - 2 * pad
        acc = None
        for j in range(K):
            acc = ops.linear_ex(flat[j:j + M], W[:, :, j].contiguous(), conv.bias.detach() if j == 0 else None, resid=acc,
                                act=3 if j == K - 1 else 0)
        out = torch.zeros(B, S + 2 * pad, d, device=x.device, dtype=torch.float32)
        out.view(-1, d)[:M] = acc
        return out[:, :S].contiguous().view(B * S, d)

    def _conv_taps(self):
        """CNN_GRU's convolution weight as autograd.ConvSiluFn's GEMMs read it: per tap j the contiguous W[:, :, j], and per tap its
        transpose (the backward's dx); rebuilt when the weight changes."""
        conv = self.model.cnn[0]

        def build():
            W = conv.weight.detach()
            K = W.shape[2]
            return tuple(W[:, :, j].contiguous() for j in range(K)), tuple(W[:, :, j].t().contiguous() for j in range(K))

        return self._tables.get("conv7", [conv.weight], build, wait=not self.training or not self._train_path())

    def _rnn_layer(self, l):
        """(W_ih, b_ih, W_hh, b_hh) of layer l with the directions stacked along the rows; rebuilt when a parameter changes."""
        names = [n + f"_l{l}" + sfx for sfx in (("", "_reverse") if self._dirs == 2 else ("",))
                 for n in ("weight_ih", "bias_ih", "weight_hh", "bias_hh")]
        ps = [getattr(self._rnn_mod, n) for n in names]

        def build():
            per = [[q.detach() for q in ps[4 * r:4 * r + 4]] for r in range(self._dirs)]
            return tuple(torch.cat([per[r][k] for r in range(self._dirs)]).contiguous() for k in range(4))

        return self._tables.get(("rnn", l), ps, build, wait=not self.training or not self._train_path())

    def _mamba(self, x, m, wdt, wx, B, L, resid, reverse):
        """MambaBlock.forward on rows x (B*L, d) + the layer's residual add (out_proj epilogue)."""
        R, N = m.dt_rank, m.d_state
        if R + 2 * N < 32:
            raise ValueError("dt_rank + 2*d_state < 32 is not supported")
        xz = ops.linear_ex(x, m.in_proj.weight.detach(), m.in_proj.bias.detach())
        xc = ops.dwconv1d_silu(xz, m.d_inner, m.conv1d.weight.detach().reshape(m.d_inner, m.d_conv).contiguous(),
                               m.conv1d.bias.detach(), B, L, reverse)
        dbc = ops.linear_ex(xc, wx)
        draw = ops.linear_ex(dbc, wdt, K=32)
        g = ops.selective_scan(xc, draw, m.dt_proj.bias.detach(), m.A_log.detach(), dbc, R, m.D.detach(), xz, B, L,
                               version=self._version, reverse=reverse)
        return ops.linear_ex(g, m.out_proj.weight.detach(), m.out_proj.bias.detach(), resid=resid)

    def _train_path(self):
        """The state in which the four recurrent regModels, 'bimamba+' / 'bimamba' and the two mixture heads build an autograd graph
        (video2music_amd/autograd.py), and after `enable_training()` the five of OPT_IN_TRAINABLE too; every other state and regModel
        runs the inference kernels on detached parameters."""
        if not (self.training and torch.is_grad_enabled()):
            return False
        return (self.regModel in ("lstm", "bilstm", "gru", "bigru", "bimamba+", "bimamba", "moe_bimamba+", "sharedmoe_bimamba+")
                or (self._training_enabled and self.regModel in self.OPT_IN_TRAINABLE))

    def _get_feature_train(self, vf, B, S, Win, Wdt, Wx):
        """get_feature's recurrent and bidirectional-Mamba branches through the autograd Functions, on the module's own parameters.
        Dropout sits where the reference has it: after in_proj (:169); between the recurrent layers, not after the last (nn.LSTM /
        nn.GRU); in a BiMambaEncoderLayer_V1 (bimamba.py:166-189) after the forward block, after the backward block, inside the FFN
        (width d_hidden) and after it; in a BiMambaEncoderLayer (:65-98) after the forward block, inside and after ffn1, after the
        backward block, inside and after ffn2.  MambaBlock constructs a Dropout of its own and never applies it (mamba.py:167,
        259-290): none here.  The multipliers (0 or 1 / (1 - p), shape (B*S, width)) are drawn by torch on the device, or taken in
        this order from `self.dropout_masks` when that is a list; the ones used are kept in `self.last_dropout_masks`.  Where no
        mask intervenes the launches are those of the inference path (residuals in the GEMM epilogues): at dropout 0 the result is
        the same bits.

        After `enable_training()`: 'mamba' / 'mamba+' have the one site after in_proj (mamba.py's ResidualBlock has none); 'moemamba'
        has it and then, per layer, the mixture layer's own sites in `dropout_rates()` order (inside the experts, on the chosen
        experts' outputs, inside the shared expert), none after the mixture (ResidualMoE, mamba.py:117-129); 'cnngru' / 'cnnbigru'
        have it, then the one after the convolution front's SiLU (CNN_GRU.cnn[2]), then the ones between the GRU layers."""
        from .. import autograd as AG
        given = list(self.dropout_masks) if self.dropout_masks is not None else None
        used = []

        def drop(x, p):
            if p <= 0.0:
                return x
            mask = given.pop(0) if given is not None else AG.dropout_mask(x.shape, p, x.device)
            used.append(mask)
            return x * mask

        drop.given, drop.used = given, used       # a mixture layer takes its own masks from, and leaves them in, the same two lists

        lin = self.in_proj[0]
        x = drop(AG.LinearFn.apply(vf, lin.weight, lin.bias, 0, Win), self.in_proj[1].p)
        if not self._rnn:
            x = (self._bimamba_train if self._bidirectional else self._mamba_stack_train)(x, B, S, drop, Wdt, Wx)
            self.__dict__["last_dropout_masks"] = used
            return x.view(B, S, self.d_model)
        if self._rnn_mod is not self.model:          # CNN_GRU.cnn: Conv1d + SiLU + Dropout
            conv = self.model.cnn[0]
            x = drop(AG.ConvSiluFn.apply(x, B, S, conv.weight, conv.bias, self._conv_taps()), self.model.cnn[2].p)
        gates = 4 if isinstance(self._rnn_mod, nn.LSTM) else 3
        for l in range(self.n_layers):
            names = [n + f"_l{l}" + sfx for sfx in (("", "_reverse") if self._dirs == 2 else ("",))
                     for n in ("weight_ih", "bias_ih", "weight_hh", "bias_hh")]
            x = AG.RnnLayerFn.apply(x, B, S, gates, False, self._rnn_layer(l), *[getattr(self._rnn_mod, n) for n in names])
            if l < self.n_layers - 1:
                x = drop(x, self._rnn_mod.dropout)
        self.__dict__["last_dropout_masks"] = used
        return x.view(B, S, self._dirs * self.d_model)

    def _mamba_stack_train(self, x, B, S, drop, Wdt, Wx):
        """The layers of 'mamba' / 'mamba+' (x = MambaBlock(RMSNorm(x)) + x, the sum in the out-projection's epilogue) and of 'moemamba'
        (then x = moe_layer(RMSNorm(x)) + x) on the graph.  The mixture layer takes its masks from, and leaves them in, `drop`'s lists."""
        from .. import autograd as AG
        for i, lyr in enumerate(self.model.layers):
            blk = lyr[0] if isinstance(lyr, nn.Sequential) else lyr
            m = blk.mixer
            if m.dt_rank + 2 * m.d_state < 32:
                raise ValueError("dt_rank + 2*d_state < 32 is not supported")
            h = AG.RMSNormFn.apply(x, None, blk.norm.weight, blk.norm.eps)
            x = AG.MambaBlockFn.apply(h, x, B, S, self._version, False, Wdt[i], Wx[i], m.in_proj.weight, m.in_proj.bias, m.conv1d.weight,
                                      m.conv1d.bias, m.x_proj.weight, m.dt_proj.weight, m.dt_proj.bias, m.A_log, m.D, m.out_proj.weight,
                                      m.out_proj.bias)
            if blk is not lyr:
                layer = lyr[1].moe_layer
                h = AG.RMSNormFn.apply(x, None, lyr[1].norm.weight, lyr[1].norm.eps)
                n = sum(q > 0.0 for q in layer.dropout_rates())
                layer.dropout_masks = [drop.given.pop(0) for _ in range(n)] if drop.given is not None else None
                f = layer(h.view(B, S, self.d_model)).reshape(B * S, self.d_model)
                layer.dropout_masks = None
                drop.used.extend(layer.last_dropout_masks)
                x = f + x
        return x

    def _bimamba_train(self, x, B, S, drop, Wdt, Wx):
        """The encoder layers of 'bimamba+' (V1) / 'bimamba' (V0) on the graph; `drop(x, p)` applies the next dropout mask."""
        from .. import autograd as AG

        def block(x, m, i, reverse, p):          # dropout(MambaBlock(x)) + x, the sum left to the GEMM epilogue where it can be
            args = (B, S, self._version, reverse, Wdt[i], Wx[i], m.in_proj.weight, m.in_proj.bias, m.conv1d.weight,
                    m.conv1d.bias, m.x_proj.weight, m.dt_proj.weight, m.dt_proj.bias, m.A_log, m.D, m.out_proj.weight, m.out_proj.bias)
            if m.dt_rank + 2 * m.d_state < 32:
                raise ValueError("dt_rank + 2*d_state < 32 is not supported")
            if p <= 0.0:
                return AG.MambaBlockFn.apply(x, x, *args), None
            return drop(AG.MambaBlockFn.apply(x, None, *args), p), x

        def ffn(x, f, resid, p_in, p_out):       # dropout(W2 dropout(relu(W1 x))) + resid, likewise
            h = drop(AG.LinearFn.apply(x, f[0].weight, f[0].bias, 1), p_in)
            if p_out <= 0.0:
                return AG.LinearFn.apply(h, f[3].weight, f[3].bias, 0, None, resid), None
            return drop(AG.LinearFn.apply(h, f[3].weight, f[3].bias), p_out), resid

        def mixture(x, layer, p_out):            # dropout(mixture(x)), the residual left to the norm; the layer's masks [inside the
            n = sum(q > 0.0 for q in layer.dropout_rates())     # experts, on their outputs, inside the shared expert] come before p_out's
            layer.dropout_masks = [drop.given.pop(0) for _ in range(n)] if drop.given is not None else None
            f = layer(x.view(B, S, self.d_model)).reshape(B * S, self.d_model)
            layer.dropout_masks = None
            drop.used.extend(layer.last_dropout_masks)
            return drop(f, p_out), x

        ln = lambda t, r, n: AG.LayerNormFn.apply(t, r, n.weight, n.bias, n.eps)
        p = self.in_proj[1].p                    # the model's one dropout rate: the encoder and its FFNs get the same (video_regression.py:159-167)
        for i, lyr in enumerate(self.model.layers):
            if self._version == 0:               # BiMambaEncoderLayer.forward
                xf = ln(*block(x, lyr.mamba_forward, 2 * i, False, p), lyr.norm1)
                xf = ln(*ffn(xf, lyr.ffn1, xf, p, p), lyr.norm2)
                xb = ln(*block(x, lyr.mamba_backward, 2 * i + 1, True, p), lyr.norm3)
                x = xf + ln(*ffn(xf, lyr.ffn2, xb, p, p), lyr.norm4)          # ffn2 reads x_f, as written at :92
            else:                                # BiMambaEncoderLayer_V1.forward, norm_first False
                xf = ln(*block(x, lyr.mamba_forward, 2 * i, False, p), lyr.norm1)
                xb = ln(*block(x, lyr.mamba_backward, 2 * i + 1, True, p), lyr.norm2)
                s = xb + xf
                x = ln(*(ffn(s, lyr.ffn, s, p, p) if isinstance(lyr.ffn, nn.Sequential) else mixture(s, lyr.ffn, p)), lyr.norm3)
        return x

    def get_feature(self, feature_semantic_list, feature_scene_offset, feature_motion, feature_emotion):
        """video_regression.py:199-238: (B, S, d_model) encoder output.  Scene offset and motion are not used."""
        Fpad, Win, Wdt, Wx = self._derived()
        dev = self.regressor.weight.device
        if dev.type != "cuda":
            raise RuntimeError("video2music_amd has no CPU path: move the module to the GPU")
        sem = feature_semantic_list.to(device=dev, dtype=torch.float32).contiguous()
        emo = feature_emotion.to(device=dev, dtype=torch.float32).contiguous()
        B, S = sem.shape[0], sem.shape[1]
        if sem.shape[2] + emo.shape[2] != self.total_vf_dim:
            raise ValueError(f"semantic ({sem.shape[2]}) + emotion ({emo.shape[2]}) features != total_vf_dim ({self.total_vf_dim})")
        vf = ops.concat2(sem.view(B * S, -1), emo.view(B * S, -1), Fpad)
        if self._train_path():
            return self._get_feature_train(vf, B, S, Win, Wdt, Wx)
        x = ops.linear_ex(vf, Win, self.in_proj[0].bias.detach())
        if self._rnn:                                   # nn.LSTM / nn.GRU (:124-135): per layer and direction, input GEMM + recurrence
            gates, d = (4 if isinstance(self._rnn_mod, nn.LSTM) else 3), self.d_model
            if self._rnn_mod is not self.model:
                x = self._conv7_silu(x, B, S)
            for l in range(self.n_layers):               # both directions: one input GEMM, one recurrence launch
                wi, bi, wh, bh = self._rnn_layer(l)
                out = torch.empty(B * S, self._dirs * d, device=dev, dtype=torch.float32)
                seq = ops.rnn_wide_seq if d > ops.RNN_NARROW_MAX else ops.rnn_seq        # the width picks the kernel
                seq(ops.linear_ex(x, wi, bi), wh, bh, out, 0, B, S, d, gates, n_dirs=self._dirs)
                x = out
            return x.view(B, S, self._dirs * d)
        if not self._bidirectional:                     # Mamba.forward (mamba.py:73-78): x = mixer(norm(x)) + x per layer
            for i, lyr in enumerate(self.model.layers):
                blk = lyr[0] if isinstance(lyr, nn.Sequential) else lyr
                h = ops.rmsnorm(x, blk.norm.weight.detach(), eps=blk.norm.eps)
                x = self._mamba(h, blk.mixer, Wdt[i], Wx[i], B, S, x, False)
                if blk is not lyr:                      # ResidualMoE: moe_layer(norm(x)) + x (mamba.py:126-128)
                    h = ops.rmsnorm(x, lyr[1].norm.weight.detach(), eps=lyr[1].norm.eps)
                    x = ops.add(lyr[1].moe_layer(h.view(B, S, self.d_model)).reshape(B * S, self.d_model), x)
            return x.view(B, S, self.d_model)
        if self._version == 0:                          # BiMambaEncoderLayer.forward (bimamba.py:61-100)
            ln = lambda t, n, post=None: ops.layernorm_post(t, n.weight.detach(), n.bias.detach(), post=post, eps=n.eps)
            ffn = lambda t, f, resid: ops.linear_ex(ops.linear_ex(t, f[0].weight.detach(), f[0].bias.detach(), act=1),
                                                    f[3].weight.detach(), f[3].bias.detach(), resid=resid)
            for i, lyr in enumerate(self.model.layers):
                xf = ln(self._mamba(x, lyr.mamba_forward, Wdt[2 * i], Wx[2 * i], B, S, x, False), lyr.norm1)
                xf = ln(ffn(xf, lyr.ffn1, xf), lyr.norm2)
                xb = ln(self._mamba(x, lyr.mamba_backward, Wdt[2 * i + 1], Wx[2 * i + 1], B, S, x, True), lyr.norm3)
                x = ln(ffn(xf, lyr.ffn2, xb), lyr.norm4, post=xf)      # ffn2 reads x_f, as written at :94; then x_f + x_b
            return x.view(B, S, self.d_model)
        for i, lyr in enumerate(self.model.layers):
            xf = ops.layernorm_post(self._mamba(x, lyr.mamba_forward, Wdt[2 * i], Wx[2 * i], B, S, x, False),
                                    lyr.norm1.weight.detach(), lyr.norm1.bias.detach(), eps=lyr.norm1.eps)
            s = ops.layernorm_post(self._mamba(x, lyr.mamba_backward, Wdt[2 * i + 1], Wx[2 * i + 1], B, S, x, True),
                                   lyr.norm2.weight.detach(), lyr.norm2.bias.detach(), post=xf, eps=lyr.norm2.eps)      # x_f + x_b
            if isinstance(lyr.ffn, nn.Sequential):
                h = ops.linear_ex(s, lyr.ffn[0].weight.detach(), lyr.ffn[0].bias.detach(), act=1)
                f, r = ops.linear_ex(h, lyr.ffn[3].weight.detach(), lyr.ffn[3].bias.detach(), resid=s), None
            else:                                       # the mixture layer in the FFN's place; the residual enters the norm
                f, r = lyr.ffn(s.view(B, S, self.d_model)).reshape(B * S, self.d_model), s
            x = ops.layernorm_post(f, lyr.norm3.weight.detach(), lyr.norm3.bias.detach(), resid=r, eps=lyr.norm3.eps)
        return x.view(B, S, self.d_model)

    def forward(self, feature_semantic_list, feature_scene_offset, feature_motion, feature_emotion):
        """-> (loudness_notedensity (B,S,2), instrument (B,S,40)) like video_regression.py:240-245."""
        out = self.get_feature(feature_semantic_list, feature_scene_offset, feature_motion, feature_emotion).contiguous()
        B, S, d = out.shape
        rows = out.view(B * S, d)
        if self._train_path():                          # the heads on the graph; `inst` carries the stand-in for its logits
            from .. import autograd as AG
            ln_nd = AG.LinearFn.apply(rows, self.regressor.weight, self.regressor.bias)
            inst, logits = AG.SigmoidHeadFn.apply(rows, self.classifier[0].weight, self.classifier[0].bias)
            inst = inst.view(B, S, INSTRUMENT_SIZE)
            inst._amt_logits = logits
            return ln_nd.view(B, S, 2), inst
        ln_nd = ops.linear_ex(rows, self.regressor.weight.detach(), self.regressor.bias.detach())
        inst = ops.linear_ex(rows, self.classifier[0].weight.detach(), self.classifier[0].bias.detach(), act=2)
        return ln_nd.view(B, S, 2), inst.view(B, S, INSTRUMENT_SIZE)
