"""TEST INFRASTRUCTURE (oracle) -- the fp32 numpy oracle with the roundings of the HIP bf16 / bf16w2 paths switched in.

The HIP bf16 path rounds to bf16 at a fixed list of points (the operands of the MFMA contractions); everything else -- residual
stream, LayerNorm statistics, local attention, conditioning -- is fp32.  `RoundedOracle` restates `MDMOracle` with one switch per
point (round to nearest even, products and sums in fp32 like the MFMA), so that its distance to the fp32 oracle is a MODEL of the
device's own error: the same roundings, another order of the sums.  tests/rowcheck.py bounds every row of a device result with it;
tests/bf16_ablation.py switches the points one at a time.

Points (`POINTS`): weights (all packed matrices; by matrix: `WPOINTS`), state (x_t as the pose embedding's operand), x0a (encoder
input into the layer-0 QKV), ln2 (LayerNorm2 rows into QKV / the pose head), qk (Q and K as stored), v (V as stored), p (softmax
numerators into the PV product), attn (attention rows into out_proj), ln1 (LayerNorm1 rows into linear1), hidden (GELU output into
linear2).

Modes:
  "bf16"    every point that is on rounds to one bf16 number (8 mantissa bits).
  "bf16w2"  the operands the kernels carry as hi + lo pairs -- hi = bf16(v), lo = bf16(v - hi), 16 mantissa bits -- are rounded to
            that pair (`PAIRS`): every packed WEIGHT (`P::wload` -> two-register `wfrag`: pose embedding, in_proj, out_proj,
            linear1, linear2, pose head) and the A operands a kernel of the step produces itself and hands to `P::mma_w` /
            `P::mma_a` as an `afrag`: ln2 (LayerNorm2 rows, `store4_a` / `aload`), attn (attention rows), ln1 (LayerNorm1 rows),
            hidden (`store4_afrag` / `aload_frag`).  Single bf16 as in the bf16 mode: state (x_t), qk, v, p -- the operands of
            plain `P::mma` -- and x0a in the LATENCY / TILE kernels; the ROWS kernels carry x0a (the embedding output) as a pair
            too: pass `pairs=PAIRS + ("x0a",)`.
With no point on (and `device_form` left alone) every method is MDMOracle's: the same bits."""
from __future__ import annotations

import math

import numpy as np

from . import mdm as M

POINTS = ["weights", "state", "x0a", "ln2", "qk", "v", "p", "attn", "ln1", "hidden"]
# "weights" by matrix (`weights` = all six): pose embedding (folded), in_proj, out_proj, linear1, linear2, pose head
WPOINTS = {"w_in": (), "w_qkv": ("in_proj_weight",), "w_o": ("out_proj.weight",), "w_1": ("linear1.weight",), "w_2": ("linear2.weight",),
           "w_out": ("poseFinal.weight",)}
PAIRS = ("weights",) + tuple(WPOINTS) + ("ln2", "attn", "ln1", "hidden")


def bf16(x):
    """fp32 -> bf16 -> fp32, round to nearest even (v_cvt_pk_bf16_f32)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16x2(x):
    """fp32 -> hi + lo bf16 pair -> fp32 (PBF16W2::split4: hi = bf16(v), lo = bf16(v - hi))."""
    x = np.ascontiguousarray(x, np.float32)
    hi = bf16(x)
    return hi + bf16(x - hi)


class RoundedOracle(M.MDMOracle):
    """MDMOracle with bf16 rounding at the points in `on`; the arithmetic between them is the oracle's.

    `device_form` (default: any point on) restates two things the way the library computes them, which move the last bits only:
    the pose embedding folded into input_process2 (dsg_hip.cpp: finalize_weights packs input_process2[:, D:2D] . poseEmbedding),
    and the softmax normalised after the PV product with the sum of the unrounded numerators."""

    def __init__(self, sd, cfg, on, mode="bf16", pairs=PAIRS, device_form=None):
        super().__init__(sd, cfg)
        assert mode in ("bf16", "bf16w2")
        self.on = set(on)
        assert self.on <= set(POINTS) | set(WPOINTS), self.on
        self.mode, self.pairs = mode, set(pairs)
        self.device_form = bool(self.on) if device_form is None else bool(device_form)
        if not self.device_form:
            assert not self.on
            return
        s = self.sd
        D = cfg.latent_dim
        W2 = s["input_process2.weight"].astype(np.float64)
        # the library folds input_process2[:, D:2D] . poseEmbedding and packs THAT
        self.Wfold = (W2[:, D:2 * D] @ s["input_process.poseEmbedding.weight"].astype(np.float64)).astype(np.float32)
        self.cbase = (W2[:, D:2 * D] @ s["input_process.poseEmbedding.bias"].astype(np.float64) + s["input_process2.bias"]).astype(np.float32)
        self.W2a, self.W2c = s["input_process2.weight"][:, :D], s["input_process2.weight"][:, 2 * D:]
        if "weights" in self.on or "w_in" in self.on:
            self.Wfold = self._round("weights", self.Wfold)
        tags = [t for w, ts in WPOINTS.items() if w in self.on or "weights" in self.on for t in ts]
        for k in list(s):
            if any(t in k for t in tags):
                s[k] = self._round("weights", s[k])

    def _round(self, name, x):
        return bf16x2(x) if self.mode == "bf16w2" and name in self.pairs else bf16(x)

    def R(self, name, x):
        return self._round(name, x) if name in self.on else x

    def _encoder_layer(self, x, i, first=False):
        if not self.device_form:
            return super()._encoder_layer(x, i)
        sd, cfg = self.sd, self.cfg
        p = f"seqTransEncoder.layers.{i}."
        B, n, D = x.shape
        H = cfg.num_heads
        hd = D // H
        qkv = M._lin(self.R("x0a" if first else "ln2", x), sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"])
        q, k, v = self.R("qk", qkv[..., :D]), self.R("qk", qkv[..., D:2 * D]), self.R("v", qkv[..., 2 * D:])
        sh = lambda t: t.reshape(B, n, H, hd).transpose(0, 2, 1, 3)
        q, k, v = sh(q), sh(k), sh(v)
        s = (q @ k.transpose(0, 1, 3, 2)) * np.float32(1.0 / math.sqrt(hd))
        e = np.exp(s - s.max(-1, keepdims=True))
        o = (self.R("p", e) @ v) / e.sum(-1, keepdims=True)          # the kernels normalise after the PV product, sum from fp32 numerators
        o = o.transpose(0, 2, 1, 3).reshape(B, n, D)
        o = M._lin(self.R("attn", o), sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])
        x = M._layer_norm(x + o, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
        hid = M._gelu(M._lin(self.R("ln1", x), sd[p + "linear1.weight"], sd[p + "linear1.bias"]))
        f = M._lin(self.R("hidden", hid), sd[p + "linear2.weight"], sd[p + "linear2.bias"])
        return M._layer_norm(x + f, sd[p + "norm2.weight"], sd[p + "norm2.bias"])

    def forward(self, x, timesteps, y, uncond_info=False):
        if not self.device_form:
            return super().forward(x, timesteps, y, uncond_info)
        cfg, sd, dt = self.cfg, self.sd, self.dt
        x = np.asarray(x).astype(dt)
        B, J, _, T = x.shape
        D, Hl = cfg.latent_dim, cfg.local_heads
        # conditioning: fp32 on the device (dsg_hip.cpp: cond_rows), the oracle's arithmetic here
        emb_t = self.timestep_embed(timesteps)
        seed = np.asarray(y["seed"]).astype(dt)
        audio = np.asarray(y["audio"]).astype(dt)
        if uncond_info:
            style_e = np.zeros((B, cfg.tok_style_dim), dt)
        else:
            style_e = M._lin(np.asarray(y["style"]).astype(dt), sd["embed_style.weight"], sd["embed_style.bias"])
        if cfg.variant == 3:
            seed_in = np.zeros((B, J * cfg.n_seed), dt) if uncond_info else seed[:, :, 0, :].reshape(B, -1)
            text = M._lin(seed_in, sd["embed_text.weight"], sd["embed_text.bias"])
            tok = np.concatenate([style_e, text], 1) + emb_t
            enc = M._lin(audio, sd["WavEncoder.audio_feature_map.weight"], sd["WavEncoder.audio_feature_map.bias"])
        else:
            parts = [M._lin(seed[:, :, 0, :].transpose(0, 2, 1), sd["embed_text.weight"], sd["embed_text.bias"]),
                     M._lin(audio, sd["WavEncoder.audio_feature_map.weight"], sd["WavEncoder.audio_feature_map.bias"])]
            if cfg.variant == 5:
                last = np.asarray(y["seed_last"]).astype(dt)
                parts.append(M._lin(last[:, :, 0, :].transpose(0, 2, 1), sd["embed_text_last.weight"], sd["embed_text_last.bias"]))
            enc = np.concatenate(parts, 1)
            tok = style_e + emb_t
        xf = x[:, :, 0, :].transpose(0, 2, 1)
        h = self.R("state", xf) @ self.Wfold.T + (tok @ self.W2a.T)[:, None, :] + enc @ self.W2c.T + self.cbase
        self.probes["after_input_process2"] = h
        hd = D // Hl
        hh = h.reshape(B, T, Hl, hd).transpose(0, 2, 1, 3).reshape(B * Hl, T, hd)
        hh = M._rotary(hh, self.inv_freq).astype(dt)
        mask = y.get("mask_local", None)
        hh = M.local_attention(hh, cfg.window, None if mask is None else np.asarray(mask).astype(bool))
        h = hh.reshape(B, Hl, T, hd).transpose(0, 2, 1, 3).reshape(B, T, D)
        self.probes["after_local_attention"] = h
        xs = np.concatenate([tok[:, None, :], h], 1)
        xh = xs.reshape(B, T + 1, Hl, hd).transpose(0, 2, 1, 3).reshape(B * Hl, T + 1, hd)
        xs = M._rotary(xh, self.inv_freq).astype(dt).reshape(B, Hl, T + 1, hd).transpose(0, 2, 1, 3).reshape(B, T + 1, D)
        self.probes["encoder_in"] = xs
        for i in range(cfg.num_layers):
            xs = self._encoder_layer(xs, i, i == 0)
            self.probes[f"after_layer{i}"] = xs
        out = M._lin(self.R("ln2", xs[:, 1:]), sd["output_process.poseFinal.weight"], sd["output_process.poseFinal.bias"])
        return np.ascontiguousarray(out.transpose(0, 2, 1))[:, :, None, :].astype(dt)

    __call__ = forward
