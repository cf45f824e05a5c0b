"""Host-side mirror of the reference's model objects for the decode path.

`DiffAudioRep` here exposes the attributes `synthesis()` touches in the reference
(srcs/sample.py:56-131): `.get_cond(wav)`, `.encoder(wav)`, `.decoder(z)`, `.quantizer(...)`,
`.diff_model(x, t, cond)`, `.diff_model.upsampling_layers` (applied in order),
`.diffusion.halfway_sampling(img, t, condition)`, `.diffusion.p_sample(x, t, cond)`.
Every one of them is a thin call into libladiffcodec.so on torch CUDA(ROCm) tensors; nothing is
computed in Python.  One `Engine` (= one ldc_ctx) holds both models of a decode session, as the
hipGraph, workspaces and step tables are shared.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np

from . import lib as L
from .spec import CodecConfig, UnetConfig, unet_graph


@dataclass
class QuantizedResult:            # reference srcs/quantization/vq.py:19-25
    quantized: "object"
    codes: "object"
    bandwidth: "object"
    penalty: Optional["object"] = None


class Engine:
    """Owns the ldc_ctx.  dtype: 'bf16' (throughput), 'f32' (exact-fp32 MFMA path, parity) or 'fp8' (bf16 activations,
    UNet conv weights as OCP fp8 e4m3 with per-output-channel scales)."""

    def __init__(self, main_codec: CodecConfig, unet: UnetConfig, cond_codec: Optional[CodecConfig] = None,
                 dtype: str = "bf16", device: int = 0, noise_seed: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("ladiffcodec_amd needs an MI355X (gfx950) GPU; no CPU fallback exists")
        self.lib = L.load()
        self.torch = torch
        self.device = torch.device("cuda", device)
        self.main_codec, self.unet, self.cond_codec = main_codec, unet, cond_codec
        cfg = L.LdcConfig()
        if dtype not in L.DTYPES:
            raise ValueError(f"dtype {dtype!r}: one of {sorted(L.DTYPES)}")
        cfg.compute_dtype = L.DTYPES[dtype]
        self.dtype = dtype
        cfg.rep_dims, cfg.n_filters = main_codec.rep_dims, main_codec.n_filters
        cfg.n_residual_layers, cfg.lstm = main_codec.n_residual_layers, main_codec.lstm
        cfg.n_enc_ratios = len(main_codec.enc_ratios)
        for i, r in enumerate(main_codec.enc_ratios):
            cfg.enc_ratios[i] = r
        cfg.diff_dims = unet.dim
        ups = list(unet.upsampling_ratios or [])
        cfg.n_upsampling_ratios = len(ups)
        for i, r in enumerate(ups):
            cfg.upsampling_ratios[i] = r
        cfg.unet_scale_cond, cfg.unet_scale_x = int(unet.unet_scale_cond), int(unet.unet_scale_x)
        cfg.has_cond_model = int(cond_codec is not None)
        cfg.cond_bandwidth = float(cond_codec.bandwidth) if cond_codec is not None else 3.0
        cfg.noise_seed = noise_seed
        if main_codec.final_activation not in L.FINAL_ACTIVATIONS:
            raise ValueError(f"final_activation {main_codec.final_activation!r}: one of {sorted(k for k in L.FINAL_ACTIVATIONS if k)}")
        if cond_codec is not None and cond_codec.final_activation != main_codec.final_activation:
            raise ValueError("both models are built with the same --final_activation (sample.py:54,63)")
        cfg.final_activation = L.FINAL_ACTIVATIONS[main_codec.final_activation]
        self._cfg = cfg
        self._ctx = C.c_void_p()
        L.check(self.lib.ldc_create(C.byref(cfg), device, C.byref(self._ctx)))
        self.stream = torch.cuda.Stream(device=self.device)
        self._finalized = False
        self._streams = []                  # open stream sessions (CodecStream)
        self._pools = []                    # open decode pools (DecodePool)

    def set_option(self, name: str, value: int) -> None:
        """ldc_set_option: 'split' (chains per batch), 'lstm_stream' (no cooperative LSTM), 'side_streams', 'fp8_act',
        'train_fp32_mfma' (training GEMMs on the exact-fp32 MFMA instead of the split-bf16 path; process-wide), 'train_bf16' (plain bf16
        products in the training GEMMs, opt-in; process-wide)."""
        L.check(self.lib.ldc_set_option(self._ctx, name.encode(), int(value)))

    def debug_raise_failure(self, code: int) -> None:
        """test hook: raise the device-side failure flag (1 = cooperative LSTM gave up, 2 = fused GroupNorm wait gave up,
        4 = LinearAttention context fold outside its valid k range)"""
        L.check(self.lib.ldc_debug_raise_failure(self._ctx, int(code)))

    def host_stats(self, reset: bool = True):
        """-> (ms inside hipGraphLaunch, ms waiting for the look-ahead window, graph replays) since the last reset"""
        a, b, n = C.c_double(), C.c_double(), C.c_int64()
        L.check(self.lib.ldc_host_stats(self._ctx, int(reset), C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def stream_info(self):
        """What the part-stream calibration measured: {'overlapping': streams of the context that run side by side with the caller's stream
        and each other (-1: no calibration yet), 'candidates', 'one_spin_ms', 'all_spin_ms', 'parts'}."""
        g, n, p = C.c_int(), C.c_int(), C.c_int()
        a, b = C.c_double(), C.c_double()
        L.check(self.lib.ldc_stream_info(self._ctx, C.byref(g), C.byref(n), C.byref(a), C.byref(b), C.byref(p)))
        return {"overlapping": g.value, "candidates": n.value, "one_spin_ms": a.value, "all_spin_ms": b.value, "parts": p.value}

    def clock_sample(self):
        """(100 MHz wall-clock ticks, shader cycles) behind everything queued on the current stream; synchronises it."""
        buf = (C.c_uint64 * 2)()
        s = self._enter()
        L.check(self.lib.ldc_clock_sample(self._ctx, buf, s))
        self._exit()
        return int(buf[0]), int(buf[1])

    def reseed(self, seed: int) -> None:
        """torch.manual_seed counterpart for the device-drawn noise: sets the Philox seed and rewinds the call counter."""
        L.check(self.lib.ldc_reseed(self._ctx, int(seed)))

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self.torch.cuda.synchronize(self.device)
            for st in list(getattr(self, "_streams", [])):      # a session holds a pointer to the context: it goes first
                st.close()
            for pool in list(getattr(self, "_pools", [])):      # (so does a decode pool)
                pool.close()
            self.lib.ldc_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- load_model(model, path, strict) : utils.py:98-108 --------------------------------------
    def load_state_dict(self, which: int, state_dict: Dict[str, np.ndarray]) -> None:
        for key, arr in state_dict.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (C.c_int64 * max(1, a.ndim))(*a.shape)
            L.check(self.lib.ldc_set_weight(self._ctx, which, key.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))

    def finalize(self, strict: bool = True) -> None:
        L.check(self.lib.ldc_finalize_weights(self._ctx, int(strict)))
        self._finalized = True

    # ---- plumbing --------------------------------------------------------------------------------
    def _f32(self, t):
        torch = self.torch
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(self.device, torch.float32).contiguous()
        return t

    def _enter(self):
        cur = self.torch.cuda.current_stream(self.device)
        if cur.cuda_stream != self.stream.cuda_stream:      # (a caller already running on the engine's stream needs no hand-over:
            self.stream.wait_stream(cur)                    # the training step makes ~1 600 calls, see DiffusionTrainer._on_engine_stream)
        return C.c_void_p(self.stream.cuda_stream)

    def _exit(self):
        cur = self.torch.cuda.current_stream(self.device)
        if cur.cuda_stream != self.stream.cuda_stream:
            cur.wait_stream(self.stream)

    def _empty(self, *shape, dtype=None):
        return self.torch.empty(*shape, device=self.device, dtype=dtype or self.torch.float32)

    # ---- stages ----------------------------------------------------------------------------------
    def encode(self, which: int, wav):
        wav = self._f32(wav)
        B, _, T = wav.shape
        hop = (self.cond_codec if which == L.MODEL_COND else self.main_codec).hop_length
        z = self._empty(B, self.main_codec.rep_dims, -(-T // hop))
        s = self._enter()
        L.check(self.lib.ldc_seanet_encode(self._ctx, which, wav.data_ptr(), B, T, z.data_ptr(), s))
        self._exit()
        return z

    def decode_latents(self, which: int, z):
        z = self._f32(z)
        B, _, Lz = z.shape
        hop = (self.cond_codec if which == L.MODEL_COND else self.main_codec).hop_length
        wav = self._empty(B, 1, Lz * hop)
        s = self._enter()
        L.check(self.lib.ldc_seanet_decode(self._ctx, which, z.data_ptr(), B, Lz, wav.data_ptr(), s))
        self._exit()
        return wav

    def rvq(self, z, n_q: int):
        z = self._f32(z)
        B, D, F = z.shape
        codes = self._empty(n_q, B, F, dtype=self.torch.int64)
        q = self._empty(B, D, F)
        s = self._enter()
        L.check(self.lib.ldc_rvq_encode(self._ctx, z.data_ptr(), B, F, n_q, codes.data_ptr(), q.data_ptr(), s))
        self._exit()
        return q, codes

    def rvq_decode(self, codes):
        codes = codes.to(self.device, self.torch.int64).contiguous()
        n_q, B, F = codes.shape
        q = self._empty(B, self.main_codec.rep_dims, F)
        s = self._enter()
        L.check(self.lib.ldc_rvq_decode(self._ctx, codes.data_ptr(), B, F, n_q, q.data_ptr(), s))
        self._exit()
        return q

    def resample(self, wav, orig_freq: int, new_freq: int = 16000):
        """torchaudio.functional.resample(wav, orig_freq, new_freq) (sample.py:84); wav [C, T] -> [C, ceil(T * new / orig)]."""
        wav = self._f32(wav)
        Cc, T = wav.shape
        out = self._empty(Cc, int(self.lib.ldc_resample_out_len(T, int(orig_freq), int(new_freq))))
        s = self._enter()
        L.check(self.lib.ldc_resample(self._ctx, wav.data_ptr(), Cc, T, int(orig_freq), int(new_freq), out.data_ptr(), s))
        self._exit()
        return out

    def get_cond(self, wav, bandwidth: float = 0.0, return_codes: bool = False):
        wav = self._f32(wav)
        B, _, T = wav.shape
        F = -(-T // self.cond_codec.hop_length)
        n_q = self.cond_codec.n_q_for_bandwidth(bandwidth if bandwidth > 0 else None)
        cond = self._empty(B, self.cond_codec.rep_dims, F)
        codes = self._empty(n_q, B, F, dtype=self.torch.int64) if return_codes else None
        s = self._enter()
        L.check(self.lib.ldc_get_cond(self._ctx, wav.data_ptr(), B, T, float(bandwidth), cond.data_ptr(),
                                      codes.data_ptr() if codes is not None else None, s))
        self._exit()
        return (cond, codes) if return_codes else cond

    def get_cond_ragged(self, wav, lengths, bandwidth: float = 0.0, return_codes: bool = False):
        """`get_cond` of items of different lengths in one call (the sender side of a ragged batch): wav [B, 1, Tmax] right-padded,
        lengths[b] samples of item b (multiples of the cond hop, 320).  Every item's rows and codes are those of `get_cond` on the item
        alone; cond [B, D, Fmax] and codes [n_q, B, Fmax] are zero behind lengths[b] // 320 frames."""
        wav = self._f32(wav)
        B, _, T = wav.shape
        lens = self._lengths(list(lengths), B)
        F = T // self.cond_codec.hop_length
        n_q = self.cond_codec.n_q_for_bandwidth(bandwidth if bandwidth > 0 else None)
        cond = self._empty(B, self.cond_codec.rep_dims, F)
        codes = self._empty(n_q, B, F, dtype=self.torch.int64) if return_codes else None
        s = self._enter()
        try:
            L.check(self.lib.ldc_get_cond_ragged(self._ctx, wav.data_ptr(), lens, B, T, float(bandwidth), cond.data_ptr(),
                                                 codes.data_ptr() if codes is not None else None, s))
        finally:
            self._exit()
        return (cond, codes) if return_codes else cond

    def open_stream(self, which: int, side: int, B: int) -> "CodecStream":
        """A stream session over one end of a SEANet codec (ldc_stream_create): B independent streams, all fresh.  Chunks pushed through
        `encode` / `decode` / `get_cond` give, joined, what the whole-sequence call gives; the first chunk of a fresh item is at least
        `min_first` long."""
        return CodecStream(self, which, side, B)

    def cond_upsample(self, cond, normalise: int = 0):
        cond = self._f32(cond)
        B, Cc, F = cond.shape
        f = int(np.prod(self.unet.upsampling_ratios or ()))
        img = self._empty(B, Cc, F * f)
        s = self._enter()
        L.check(self.lib.ldc_cond_upsample(self._ctx, cond.data_ptr(), B, F, normalise, img.data_ptr(), s))
        self._exit()
        return img

    def unet_forward(self, x, t: int, cond):
        x, cond = self._f32(x), self._f32(cond)
        B, Cx, Lx = x.shape
        eps = self._empty(B, Cx, Lx)
        s = self._enter()
        L.check(self.lib.ldc_unet_forward(self._ctx, x.data_ptr(), int(t), cond.data_ptr(), B, Lx, cond.shape[2],
                                          eps.data_ptr(), s))
        self._exit()
        return eps

    def debug_tap(self, name: str, shape):
        out = self._empty(*shape)
        s = self._enter()
        L.check(self.lib.ldc_unet_debug_tap(self._ctx, name.encode(), out.data_ptr(), out.numel(), s))
        self._exit()
        return out

    ATTN_CORE_KINDS = {"linattn": 0, "linattn_kmax_fused": 1, "linattn_ctx_tail": 2, "attn_full": 3}

    def debug_attn_core(self, kind: str, qkv, to_out=None):
        """ldc_debug_attn_core: one attention core (4 heads x 32) on qkv [B, 384, L] in the engine's UNet dtype.  kind: one of
        ATTN_CORE_KINDS; 'linattn_ctx_tail' takes to_out = (weight [C, 128], bias [C], gain [C], residual [B, C, L]) and returns
        [B, C, L], the others return [B, 128, L]."""
        qkv = self._f32(qkv)
        B, _, Lx = qkv.shape
        k = self.ATTN_CORE_KINDS[kind]
        w = b = g = r = None
        Cc = 0
        if k == 2:
            w, b, g = (np.ascontiguousarray(np.asarray(t, dtype=np.float32)) for t in to_out[:3])
            r = self._f32(to_out[3])
            Cc = int(w.shape[0])
        out = self._empty(B, Cc if k == 2 else 128, Lx)
        hp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
        s = self._enter()
        try:
            L.check(self.lib.ldc_debug_attn_core(self._ctx, k, qkv.data_ptr(), B, Lx, hp(w), hp(b), hp(g),
                                                 r.data_ptr() if r is not None else None, Cc, out.data_ptr(), s))
        finally:
            self._exit()
        return out

    def debug_attention_block(self, name: str, x):
        """ldc_debug_attention_block: the attention block 'down<i>' / 'up<i>' / 'mid' of the loaded UNet on x [B, C, L], routed by
        the plan builder under the engine's current options."""
        x = self._f32(x)
        B, _, Lx = x.shape
        out = self.torch.empty_like(x)
        s = self._enter()
        try:
            L.check(self.lib.ldc_debug_attention_block(self._ctx, name.encode(), x.data_ptr(), B, Lx, out.data_ptr(), s))
        finally:
            self._exit()
        return out

    RESNET_INFO = ("epi1", "epi2", "folded", "fuse_stats", "y_ln", "rowstat", "bm1", "wm1", "bm2", "wm2", "tags_complete", "stray_slots")

    def debug_resnet_block(self, name: str, x1, x2=None, t: int = 0, lens=None, shift: int = 0, t_items=None, with_attention=False):
        """ldc_debug_resnet_block: the ResnetBlock 'down<i>.1' / 'down<i>.2' / 'mid.1' / 'mid.2' / 'up<i>.1' / 'up<i>.2' / 'final' of the
        loaded UNet on x1 [B, cin1, L] (and x2 [B, cin2, L] where the block reads a concatenation), routed by the plan builder under
        the engine's current options.  lens (rows of level 0) with shift: a ragged plan; t_items: a per-item plan.  Returns a dict:
        out, mid (block1's stored output) [B, cout, L], stats [2, B, groups, 2] (sum, sum of squares of conv 1 / conv 2 as the kernels
        accumulated them), attn_out (with_attention: the attention block behind it), pre [2, B, cout, L] (the conv outputs as stored,
        zeros for a conv with the fused epilogue) and info (RESNET_INFO -> int)."""
        x1 = self._f32(x1)
        x2 = self._f32(x2) if x2 is not None else None
        B, _, Lx = x1.shape
        cout = self.resnet_cout(name)
        out, mid = self._empty(B, cout, Lx), self._empty(B, cout, Lx)
        attn = self._empty(B, cout, Lx) if with_attention else None
        pre = self._empty(2, B, cout, Lx)
        stats = np.zeros((2, B, self.unet.groups, 2), np.float32)
        info = (C.c_int * 12)()
        arr = lambda v: (C.c_int * B)(*[int(i) for i in v]) if v is not None else None   # noqa: E731
        s = self._enter()
        try:
            L.check(self.lib.ldc_debug_resnet_block(self._ctx, name.encode(), x1.data_ptr(), x2.data_ptr() if x2 is not None else None, B, Lx,
                                                    int(t), arr(lens), int(shift), arr(t_items), int(bool(with_attention)), out.data_ptr(),
                                                    mid.data_ptr(), stats.ctypes.data_as(C.c_void_p), attn.data_ptr() if attn is not None else None,
                                                    pre.data_ptr(), info, s))
        finally:
            self._exit()
        return dict(out=out, mid=mid, stats=stats, attn_out=attn, pre=pre, info=dict(zip(self.RESNET_INFO, info)))

    def debug_resnet_route(self, name: str, B: int, Lx: int, lens=None, shift: int = 0, per_item=False, with_attention=False):
        """the info dict of the debug_resnet_block call with these arguments, from the planner alone (nothing is launched)"""
        info = (C.c_int * 12)()
        arr = lambda v: (C.c_int * B)(*[int(i) for i in v]) if v is not None else None   # noqa: E731
        L.check(self.lib.ldc_debug_resnet_block(self._ctx, name.encode(), None, None, int(B), int(Lx), 0, arr(lens), int(shift),
                                                arr([0] * B) if per_item else None, int(bool(with_attention)), None, None, None, None, None, info, None))
        return dict(zip(self.RESNET_INFO[:10], info))

    def resnet_cout(self, name: str) -> int:
        """output channels of the ResnetBlock `name` (debug_resnet_block's names)"""
        g = unet_graph(self.unet)
        if name == "final":
            return g.final.cout
        lvl, which = name.split(".")
        if lvl == "mid":
            return (g.mid1 if which == "1" else g.mid2).cout
        lv = (g.downs if lvl.startswith("down") else g.ups)[int(lvl.lstrip("downup"))]
        return (lv.block1 if which == "1" else lv.block2).cout

    SEA_ROUTES = {1: "cin1_rows", 2: "cin1_generic", 3: "pipelined", 4: "generic"}
    SEA_OP_KINDS = ("conv_cin1", "conv", "convtr", "res", "lstm")

    def debug_sea_conv(self, x, w, b, stride=1, dilation=1, causal=True, transposed=False, pre_elu=False, residual=None):
        """ldc_debug_sea_conv: one SEANet conv (plain: w [Cout, Cin, k]; transposed: w [Cin, Cout, k], k = 2 * stride) on x [B, Cin, L]
        through the conv path of an encode / decode.  Returns (y [B, Cout, Lout], route): route = {"route": one of SEA_ROUTES' names}
        and, for the generic kernel, "tile" (WM, WN, TM, TN), "ksplit", "tg" and "bn"."""
        x = self._f32(x)
        w = np.ascontiguousarray(w, np.float32)
        b = np.ascontiguousarray(b, np.float32) if b is not None else None
        B, Cin, Lx = x.shape
        if transposed:
            _, Cout, k = w.shape
            Lout = Lx * stride
        else:
            Cout, _, k = w.shape
            Lout = -(-Lx // stride)
        r = self._f32(residual) if residual is not None else None
        y = self._empty(B, Cout, Lout)
        route = (C.c_int * 8)()
        s = self._enter()
        try:
            L.check(self.lib.ldc_debug_sea_conv(self._ctx, x.data_ptr(), B, Cin, Lx, w.ctypes.data_as(C.c_void_p),
                                                b.ctypes.data_as(C.c_void_p) if b is not None else None, Cout, k, stride, dilation,
                                                int(causal), int(transposed), int(pre_elu), r.data_ptr() if r is not None else None,
                                                y.data_ptr(), route, s))
        finally:
            self._exit()
        rep = {"route": self.SEA_ROUTES.get(route[0], "none")}
        if route[0] == 4:
            rep.update(tile=tuple(route[1:5]), ksplit=route[5], tg=route[6], bn=route[7])
        return y, rep

    def debug_sea_op_info(self, which: int, decoder: bool, index: int, B: int, Lx: int):
        """(kind, C_in, C_out, L_out) of op `index` of the loaded codec's encoder / decoder for an input of Lx positions."""
        info = (C.c_int * 4)()
        L.check(self.lib.ldc_debug_sea_op(self._ctx, which, int(decoder), index, None, B, Lx, None, 0, info, None))
        return self.SEA_OP_KINDS[info[0]], info[1], info[2], info[3]

    def debug_sea_op(self, which: int, decoder: bool, index: int, x):
        """ldc_debug_sea_op: op `index` of the encoder / decoder of the loaded codec `which` alone on x [B, C_in, L]."""
        x = self._f32(x)
        B, _, Lx = x.shape
        _, _, Co, Lo = self.debug_sea_op_info(which, decoder, index, B, Lx)
        out = self._empty(B, Co, Lo)
        info = (C.c_int * 4)()
        s = self._enter()
        try:
            L.check(self.lib.ldc_debug_sea_op(self._ctx, which, int(decoder), index, x.data_ptr(), B, Lx, out.data_ptr(), out.numel(), info, s))
        finally:
            self._exit()
        return out

    def p_sample(self, x, t: int, cond, noise=None):
        x = self._f32(x).clone()
        cond = self._f32(cond)
        noise = self._f32(noise) if noise is not None else None
        B, _, Lx = x.shape
        s = self._enter()
        L.check(self.lib.ldc_p_sample(self._ctx, x.data_ptr(), int(t), cond.data_ptr(),
                                      noise.data_ptr() if noise is not None else None, B, Lx, cond.shape[2], s))
        self._exit()
        return x

    def denoise(self, img, cond, n_steps: int, noise=None, inplace: bool = False):
        img = self._f32(img)
        if not inplace:
            img = img.clone()
        cond = self._f32(cond)
        noise = self._f32(noise) if noise is not None else None
        B, _, Lx = img.shape
        s = self._enter()
        L.check(self.lib.ldc_denoise(self._ctx, img.data_ptr(), cond.data_ptr(),
                                     noise.data_ptr() if noise is not None else None, int(n_steps), B, Lx, cond.shape[2], s))
        self._exit()
        return img

    def p_sample_loop(self, cond, img=None, noise=None, length: Optional[int] = None):
        """diffusion.p_sample_loop: all `timesteps` ancestral steps from `img` (or from a device-drawn N(0,1) image)."""
        cond = self._f32(cond)
        B, _, F = cond.shape
        if img is None:
            Lx = int(length) if length is not None else F * int(np.prod(self.unet.upsampling_ratios or ()))
            img = self.torch.empty(B, self.unet.inp_channels, Lx, device=cond.device, dtype=self.torch.float32)
            fill = 1
        else:
            img = self._f32(img).clone()
            fill = 0
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        L.check(self.lib.ldc_p_sample_loop(self._ctx, img.data_ptr(), cond.data_ptr(),
                                           noise.data_ptr() if noise is not None else None, fill, B, img.shape[2], F, s))
        self._exit()
        return img

    def infilling(self, infill_img, cond, midway_t: int, lam: float = 0.8, img=None, noise=None):
        """diffusion.infilling; returns (img, infill_img) after the loop (the reference returns img)."""
        cond = self._f32(cond)
        infill = self._f32(infill_img).clone()
        B, _, Lx = infill.shape
        if img is None:
            img = self.torch.empty_like(infill)
            fill = 1
        else:
            img = self._f32(img).clone()
            fill = 0
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        L.check(self.lib.ldc_infilling(self._ctx, img.data_ptr(), infill.data_ptr(), cond.data_ptr(), int(midway_t),
                                       noise.data_ptr() if noise is not None else None, float(lam), fill, B, Lx, cond.shape[2], s))
        self._exit()
        return img, infill

    def ddim_sample(self, cond, t_start: int, n_steps: int, eta: float = 0.0, img=None, noise=None, length: Optional[int] = None):
        """DDIM sampling (diffusion.ddim_sample with clip_denoised) from `t_start`: n_steps strided iterations from `img` (or from a
        device-drawn N(0,1) image).  noise [n_steps, B, C, L] injects the draws (parity runs)."""
        cond = self._f32(cond)
        B, _, F = cond.shape
        if img is None:
            Lx = int(length) if length is not None else F * int(np.prod(self.unet.upsampling_ratios or ()))
            img = self.torch.empty(B, self.unet.inp_channels, Lx, device=cond.device, dtype=self.torch.float32)
            fill = 1
        else:
            img = self._f32(img).clone()
            fill = 0
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        L.check(self.lib.ldc_ddim_sample(self._ctx, img.data_ptr(), cond.data_ptr(), noise.data_ptr() if noise is not None else None,
                                         fill, int(t_start), int(n_steps), float(eta), B, img.shape[2], F, s))
        self._exit()
        return img

    def dpm_sample(self, cond, t_start: int, n_steps: int, img):
        """DPM-Solver++(2M) sampling (data-prediction form, clipped x0) from `t_start`: n_steps iterations on DDIM's timestep list
        from `img`.  Deterministic: nothing is drawn and the engine's noise epoch stays where it is."""
        cond = self._f32(cond)
        B, _, F = cond.shape
        if img is None:
            raise ValueError("dpm_sample takes its start image from the caller (there is no device-drawn one)")
        img = self._f32(img).clone()
        s = self._enter()
        try:
            L.check(self.lib.ldc_dpm_sample(self._ctx, img.data_ptr(), cond.data_ptr(), int(t_start), int(n_steps), B, img.shape[2], F, s))
        finally:
            self._exit()
        return img

    def output_normalise(self, wav, per_item: bool = False):
        wav = self._f32(wav).clone()
        B = wav.shape[0]
        s = self._enter()
        L.check(self.lib.ldc_output_normalise(self._ctx, wav.data_ptr(), B, wav.numel() // B, int(per_item), s))
        self._exit()
        return wav

    def decode(self, wav, n_steps: int, noise=None, per_item: bool = False, want_stages: bool = False):
        """The per-batch body of synthesis() (sample.py:94-134) in one library call."""
        wav = self._f32(wav)
        B, _, T = wav.shape
        F, Lz = T // self.cond_codec.hop_length, T // self.main_codec.hop_length
        out = self._empty(B, 1, T)
        lat = self._empty(B, self.main_codec.rep_dims, Lz) if want_stages else None
        cond = self._empty(B, self.main_codec.rep_dims, F) if want_stages else None
        n_q = self.cond_codec.n_q_for_bandwidth(None)
        codes = self._empty(n_q, B, F, dtype=self.torch.int64) if want_stages else None
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        p = lambda t: t.data_ptr() if t is not None else None
        L.check(self.lib.ldc_decode(self._ctx, wav.data_ptr(), B, T, int(n_steps), p(noise), int(per_item), out.data_ptr(),
                                    p(lat), p(cond), p(codes), s))
        self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond, "codes": codes}
        return out

    def decode_ddim(self, wav, t_start: int, n_steps: int, eta: float = 0.0, noise=None, per_item: bool = False,
                    want_stages: bool = False):
        """`decode` with DDIM sampling: n_steps iterations from t_start, starting at the upsampled, normalised condition."""
        wav = self._f32(wav)
        B, _, T = wav.shape
        F, Lz = T // self.cond_codec.hop_length, T // self.main_codec.hop_length
        out = self._empty(B, 1, T)
        lat = self._empty(B, self.main_codec.rep_dims, Lz) if want_stages else None
        cond = self._empty(B, self.main_codec.rep_dims, F) if want_stages else None
        n_q = self.cond_codec.n_q_for_bandwidth(None)
        codes = self._empty(n_q, B, F, dtype=self.torch.int64) if want_stages else None
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        p = lambda t: t.data_ptr() if t is not None else None
        L.check(self.lib.ldc_decode_ddim(self._ctx, wav.data_ptr(), B, T, int(t_start), int(n_steps), float(eta), p(noise),
                                         int(per_item), out.data_ptr(), p(lat), p(cond), p(codes), s))
        self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond, "codes": codes}
        return out

    def decode_dpm(self, wav, t_start: int, n_steps: int, per_item: bool = False, want_stages: bool = False):
        """`decode` with DPM-Solver++(2M) sampling: n_steps iterations from t_start, starting at the upsampled, normalised condition."""
        wav = self._f32(wav)
        B, _, T = wav.shape
        F, Lz = T // self.cond_codec.hop_length, T // self.main_codec.hop_length
        out = self._empty(B, 1, T)
        lat = self._empty(B, self.main_codec.rep_dims, Lz) if want_stages else None
        cond = self._empty(B, self.main_codec.rep_dims, F) if want_stages else None
        n_q = self.cond_codec.n_q_for_bandwidth(None)
        codes = self._empty(n_q, B, F, dtype=self.torch.int64) if want_stages else None
        s = self._enter()
        p = lambda t: t.data_ptr() if t is not None else None
        try:
            L.check(self.lib.ldc_decode_dpm(self._ctx, wav.data_ptr(), B, T, int(t_start), int(n_steps), int(per_item), out.data_ptr(),
                                            p(lat), p(cond), p(codes), s))
        finally:
            self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond, "codes": codes}
        return out

    @staticmethod
    def _lengths(lengths, B: int):
        arr = (C.c_int32 * B)(*[int(v) for v in lengths])
        if len(lengths) != B:
            raise ValueError(f"{len(lengths)} lengths for a batch of {B}")
        return arr

    def decode_ragged(self, wav, lengths, n_steps: int, t_start: int = 0, eta: float = 0.0, noise=None, want_stages: bool = False):
        """`decode` (t_start 0) / `decode_ddim` (t_start > 0) of items of different lengths in one call: wav [B, 1, Tmax] right-padded,
        lengths[b] samples of item b (multiples of the chunk quantum, sample.chunk_quantum).  Every item comes out as if decoded
        alone (per-item normalisation); item b consumes noise[:, b, :, :L_b]; outputs are zero beyond an item's length."""
        wav = self._f32(wav)
        B, _, T = wav.shape
        F, Lz = T // self.cond_codec.hop_length, T // self.main_codec.hop_length
        lens = self._lengths(list(lengths), B)
        out = self._empty(B, 1, T)
        lat = self._empty(B, self.main_codec.rep_dims, Lz) if want_stages else None
        cond = self._empty(B, self.main_codec.rep_dims, F) if want_stages else None
        n_q = self.cond_codec.n_q_for_bandwidth(None)
        codes = self._empty(n_q, B, F, dtype=self.torch.int64) if want_stages else None
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        p = lambda t: t.data_ptr() if t is not None else None
        try:
            L.check(self.lib.ldc_decode_ragged(self._ctx, wav.data_ptr(), lens, B, T, int(t_start), int(n_steps), float(eta), p(noise),
                                               out.data_ptr(), p(lat), p(cond), p(codes), s))
        finally:
            self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond, "codes": codes}
        return out

    def decode_ragged_dpm(self, wav, lengths, t_start: int, n_steps: int, want_stages: bool = False):
        """`decode_dpm` of items of different lengths in one call (the layout and rules of `decode_ragged`): every item comes out as
        if decoded alone, outputs are zero beyond an item's length."""
        wav = self._f32(wav)
        B, _, T = wav.shape
        F, Lz = T // self.cond_codec.hop_length, T // self.main_codec.hop_length
        lens = self._lengths(list(lengths), B)
        out = self._empty(B, 1, T)
        lat = self._empty(B, self.main_codec.rep_dims, Lz) if want_stages else None
        cond = self._empty(B, self.main_codec.rep_dims, F) if want_stages else None
        n_q = self.cond_codec.n_q_for_bandwidth(None)
        codes = self._empty(n_q, B, F, dtype=self.torch.int64) if want_stages else None
        s = self._enter()
        p = lambda t: t.data_ptr() if t is not None else None
        try:
            L.check(self.lib.ldc_decode_ragged_dpm(self._ctx, wav.data_ptr(), lens, B, T, int(t_start), int(n_steps), out.data_ptr(),
                                                   p(lat), p(cond), p(codes), s))
        finally:
            self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond, "codes": codes}
        return out

    def unet_forward_ragged(self, x, t: int, cond, latent_lens):
        """`unet_forward` with per-item latent lengths: x [B, C, Lmax], cond [B, C, Fmax]; eps is zero beyond an item's length."""
        x, cond = self._f32(x), self._f32(cond)
        B, Cx, Lx = x.shape
        lens = self._lengths(list(latent_lens), B)
        eps = self._empty(B, Cx, Lx)
        s = self._enter()
        try:
            L.check(self.lib.ldc_unet_forward_ragged(self._ctx, x.data_ptr(), int(t), cond.data_ptr(), lens, B, Lx, cond.shape[2],
                                                     eps.data_ptr(), s))
        finally:
            self._exit()
        return eps

    # ---- coupled windows: one long recording on one shared latent ----------
    def window_layout(self, Ltot: int, Lw: int, overlap: int):
        """ldc_window_layout for this engine's `up`: -> (starts [W], weights [W, min(Lw, Ltot)] float32)."""
        return L.window_layout(Ltot, Lw, overlap, int(np.prod(self.unet.upsampling_ratios or ())))

    def _one_recording(self, x, what: str):
        x = self._f32(x)
        if x.dim() != 3 or x.shape[0] != 1:
            raise ValueError(f"{what}: coupled windows take one recording per call ([1, C, L]), got {tuple(x.shape)}")
        return x

    def unet_forward_windows(self, x, t: int, cond, Lw: int, overlap: int):
        """The blended eps of one UNet pass over the windows of x [1, C, Ltot] (cond [1, C, Ftot], raw): [1, C, Ltot]."""
        x, cond = self._one_recording(x, "x"), self._one_recording(cond, "cond")
        eps = self.torch.empty_like(x)
        s = self._enter()
        try:
            L.check(self.lib.ldc_unet_forward_windows(self._ctx, x.data_ptr(), int(t), cond.data_ptr(), x.shape[2], cond.shape[2], int(Lw),
                                                      int(overlap), eps.data_ptr(), s))
        finally:
            self._exit()
        return eps

    def denoise_windows(self, img, cond, n_steps: int, Lw: int, overlap: int, noise=None):
        """`denoise` of one recording [1, C, Ltot] on coupled windows of Lw frames overlapping by `overlap`; noise [n_steps, 1, C, Ltot]."""
        img, cond = self._one_recording(img, "img").clone(), self._one_recording(cond, "cond")
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        try:
            L.check(self.lib.ldc_denoise_windows(self._ctx, img.data_ptr(), cond.data_ptr(), noise.data_ptr() if noise is not None else None,
                                                 int(n_steps), img.shape[2], cond.shape[2], int(Lw), int(overlap), s))
        finally:
            self._exit()
        return img

    def ddim_sample_windows(self, img, cond, t_start: int, n_steps: int, Lw: int, overlap: int, eta: float = 0.0, noise=None):
        """`ddim_sample` (from the caller's start image) of one recording on coupled windows."""
        img, cond = self._one_recording(img, "img").clone(), self._one_recording(cond, "cond")
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        try:
            L.check(self.lib.ldc_ddim_sample_windows(self._ctx, img.data_ptr(), cond.data_ptr(), noise.data_ptr() if noise is not None else None,
                                                     int(t_start), int(n_steps), float(eta), img.shape[2], cond.shape[2], int(Lw),
                                                     int(overlap), s))
        finally:
            self._exit()
        return img

    def _decode_windows(self, wav, want_stages: bool, call):
        wav = self._one_recording(wav, "wav")
        T = wav.shape[2]
        F, Lz = T // self.cond_codec.hop_length, T // self.main_codec.hop_length
        out = self._empty(1, 1, T)
        lat = self._empty(1, self.main_codec.rep_dims, Lz) if want_stages else None
        cond = self._empty(1, self.main_codec.rep_dims, F) if want_stages else None
        codes = self._empty(self.cond_codec.n_q_for_bandwidth(None), 1, F, dtype=self.torch.int64) if want_stages else None
        p = lambda t: t.data_ptr() if t is not None else None
        s = self._enter()
        try:
            L.check(call(wav.data_ptr(), T, out.data_ptr(), p(lat), p(cond), p(codes), s))
        finally:
            self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond, "codes": codes}
        return out

    def decode_windows(self, wav, n_steps: int, Lw: int, overlap: int, noise=None, want_stages: bool = False):
        """`decode` of one recording wav [1, 1, T] with the denoise loop on coupled windows (Lw, overlap in latent frames)."""
        noise = self._f32(noise) if noise is not None else None
        pn = noise.data_ptr() if noise is not None else None
        return self._decode_windows(wav, want_stages, lambda w, T, o, la, co, cd, s: self.lib.ldc_decode_windows(
            self._ctx, w, T, int(n_steps), pn, int(Lw), int(overlap), o, la, co, cd, s))

    def decode_ddim_windows(self, wav, t_start: int, n_steps: int, Lw: int, overlap: int, eta: float = 0.0, noise=None,
                            want_stages: bool = False):
        """`decode_ddim` of one recording with the loop on coupled windows."""
        noise = self._f32(noise) if noise is not None else None
        pn = noise.data_ptr() if noise is not None else None
        return self._decode_windows(wav, want_stages, lambda w, T, o, la, co, cd, s: self.lib.ldc_decode_ddim_windows(
            self._ctx, w, T, int(t_start), int(n_steps), float(eta), pn, int(Lw), int(overlap), o, la, co, cd, s))

    def dpm_sample_windows(self, img, cond, t_start: int, n_steps: int, Lw: int, overlap: int):
        """`dpm_sample` (from the caller's start image) of one recording on coupled windows: ONE state, ONE x0 history.  Deterministic:
        nothing is drawn and the engine's noise epoch stays where it is."""
        img, cond = self._one_recording(img, "img").clone(), self._one_recording(cond, "cond")
        s = self._enter()
        try:
            L.check(self.lib.ldc_dpm_sample_windows(self._ctx, img.data_ptr(), cond.data_ptr(), int(t_start), int(n_steps), img.shape[2],
                                                    cond.shape[2], int(Lw), int(overlap), s))
        finally:
            self._exit()
        return img

    def decode_dpm_windows(self, wav, t_start: int, n_steps: int, Lw: int, overlap: int, want_stages: bool = False):
        """`decode_dpm` of one recording with the loop on coupled windows."""
        return self._decode_windows(wav, want_stages, lambda w, T, o, la, co, cd, s: self.lib.ldc_decode_dpm_windows(
            self._ctx, w, T, int(t_start), int(n_steps), int(Lw), int(overlap), o, la, co, cd, s))

    # ---- window groups ("Several recordings per call"): lists of recordings in, lists out ----------
    SAMPLERS = {"ddpm": 0, "ddim": 1, "dpm": 2}

    def window_group_layout(self, Ltot, Lw: int, overlap: int):
        """ldc_window_group_layout for this engine's `up`: -> (w0 [R + 1], starts [W_sum], weights [W_sum, Lw] float32)."""
        return L.window_group_layout(Ltot, Lw, overlap, int(np.prod(self.unet.upsampling_ratios or ())))

    def _pack(self, xs, what: str):
        """a list of [1, C, n_r] tensors as one packed float32 buffer of [C][n_r] blocks, and the n_r"""
        xs = [self._one_recording(x, what) for x in xs]
        if not xs:
            raise ValueError(f"{what}: a window group holds at least one recording")
        return self.torch.cat([x.reshape(-1) for x in xs]).contiguous(), [int(x.shape[2]) for x in xs]

    def _unpack(self, flat, C_: int, lens):
        out, o = [], 0
        for n in lens:
            out.append(flat[o:o + C_ * n].reshape(1, C_, n).clone())
            o += C_ * n
        return out

    @staticmethod
    def _ints(v):
        return (C.c_int * len(v))(*[int(a) for a in v])

    def _group_noise(self, noise, seeds, lens, n_rows):
        """a list of per-recording tapes [n, 1, C, Ltot_r] -> one packed tape [n][C * Lsum]; seeds -> uint64 [R]"""
        pn = ps = None
        if noise is not None:
            if len(noise) != len(lens):
                raise ValueError("noise: one tape per recording")
            tapes = [self._f32(t) for t in noise]
            n = tapes[0].shape[0]
            if any(t.dim() != 4 or t.shape[0] != n or t.shape[1] != 1 or t.shape[3] != l for t, l in zip(tapes, lens)) or n < n_rows:
                raise ValueError("noise: tapes of [n_steps, 1, C, Ltot_r], the same n_steps for every recording")
            pn = self.torch.cat([t.reshape(n, -1) for t in tapes], dim=1).contiguous()
        if seeds is not None:
            if len(seeds) != len(lens):
                raise ValueError("seeds: one per recording")
            ps = (C.c_uint64 * len(lens))(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds])
        return pn, ps

    def unet_forward_windows_group(self, xs, t: int, conds, Lw: int, overlap: int):
        """The blended eps of ONE UNet pass over the windows of every recording: xs [1, C, Ltot_r], conds [1, C, Ftot_r] (raw) -> a list
        of [1, C, Ltot_r]."""
        x, lens = self._pack(xs, "x")
        cond, flens = self._pack(conds, "cond")
        if len(lens) != len(flens):
            raise ValueError("one condition per recording")
        eps = self.torch.empty_like(x)
        s = self._enter()
        try:
            L.check(self.lib.ldc_unet_forward_windows_group(self._ctx, x.data_ptr(), int(t), cond.data_ptr(), len(lens), self._ints(lens),
                                                            self._ints(flens), int(Lw), int(overlap), eps.data_ptr(), s))
        finally:
            self._exit()
        return self._unpack(eps, xs[0].shape[1], lens)

    def sample_windows_group(self, imgs, conds, n_steps: int, Lw: int, overlap: int, sampler: str = "ddpm", t_start: int = 0,
                             eta: float = 0.0, noise=None, seeds=None):
        """`denoise_windows` ("ddpm"), `ddim_sample_windows` ("ddim") or `dpm_sample_windows` ("dpm") of every recording in ONE loop whose
        batch holds the windows of all of them (at most 32).  imgs [1, C, Ltot_r], conds [1, C, Ftot_r]; noise: a list of tapes
        [n_steps, 1, C, Ltot_r], or seeds: one per recording -- recording r then draws what the single call draws right after
        reseed(seeds[r]); the engine's own noise epoch is neither read nor advanced.  -> a list of [1, C, Ltot_r]."""
        img, lens = self._pack(imgs, "img")
        cond, flens = self._pack(conds, "cond")
        if len(lens) != len(flens):
            raise ValueError("one condition per recording")
        pn, ps = self._group_noise(noise, seeds, lens, int(n_steps))
        s = self._enter()
        try:
            L.check(self.lib.ldc_sample_windows_group(self._ctx, img.data_ptr(), cond.data_ptr(), self.SAMPLERS[sampler], int(t_start),
                                                      int(n_steps), float(eta), pn.data_ptr() if pn is not None else None, ps, len(lens),
                                                      self._ints(lens), self._ints(flens), int(Lw), int(overlap), s))
        finally:
            self._exit()
        return self._unpack(img, imgs[0].shape[1], lens)

    def decode_windows_group(self, wavs, n_steps: int, Lw: int, overlap: int, sampler: str = "ddpm", t_start: int = 0, eta: float = 0.0,
                             noise=None, seeds=None, want_stages: bool = False):
        """`decode_windows` / `decode_ddim_windows` / `decode_dpm_windows` of every recording wavs[r] [1, 1, T_r] with ONE denoise loop; the
        codec ends run per recording.  -> a list of waveforms [1, 1, T_r], or of the stage dicts of `decode_windows`."""
        wav, Ts = self._pack(wavs, "wav")
        hop_c, hop_m, D = self.cond_codec.hop_length, self.main_codec.hop_length, self.main_codec.rep_dims
        Fs, Ls = [T // hop_c for T in Ts], [T // hop_m for T in Ts]
        pn, ps = self._group_noise(noise, seeds, Ls, int(n_steps))
        n_q = self.cond_codec.n_q_for_bandwidth(None)
        out = self._empty(sum(Ts))
        lat = self._empty(D * sum(Ls)) if want_stages else None
        cond = self._empty(D * sum(Fs)) if want_stages else None
        codes = self._empty(n_q * sum(Fs), dtype=self.torch.int64) if want_stages else None
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        s = self._enter()
        try:
            L.check(self.lib.ldc_decode_windows_group(self._ctx, wav.data_ptr(), len(Ts), self._ints(Ts), self.SAMPLERS[sampler], int(t_start),
                                                      int(n_steps), float(eta), p(pn), ps, int(Lw), int(overlap), out.data_ptr(), p(lat),
                                                      p(cond), p(codes), s))
        finally:
            self._exit()
        outs = self._unpack(out, 1, Ts)
        if not want_stages:
            return outs
        lats, conds = self._unpack(lat, D, Ls), self._unpack(cond, D, Fs)
        cds, o = [], 0
        for F in Fs:
            cds.append(codes[o:o + n_q * F].reshape(n_q, 1, F).clone())
            o += n_q * F
        return [{"wav": w, "latents": a, "cond": b, "codes": cd} for w, a, b, cd in zip(outs, lats, conds, cds)]

    def _decode_codes_windows(self, codes, packed, bits, n_q, F, want_stages: bool, call):
        if codes is not None and (codes.dim() != 3 or codes.shape[1] != 1):
            raise ValueError(f"codes: coupled windows take one recording per call ([n_q, 1, F]), got {tuple(codes.shape)}")
        cp, pp, stride, n_q, B, F, keep = self._codes_args(codes, packed, bits, n_q, F)
        if B != 1:
            raise ValueError(f"packed: coupled windows take one recording per call ([1, bytes]), got {B} rows")
        out, lat, cond = self._codes_outputs(1, F, want_stages)
        p = lambda t: t.data_ptr() if t is not None else None
        s = self._enter()
        try:
            L.check(call(cp, pp, stride, int(bits), n_q, F, out.data_ptr(), p(lat), p(cond), s))
        finally:
            self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond}
        return out

    def decode_codes_windows(self, codes=None, packed=None, n_steps: Optional[int] = None, Lw: Optional[int] = None,
                             overlap: Optional[int] = None, t_start: int = 0, eta: float = 0.0, noise=None, want_stages: bool = False,
                             bits: int = 10, n_q: Optional[int] = None, F: Optional[int] = None):
        """`decode_windows` (t_start 0) / `decode_ddim_windows` (t_start > 0) started from the RVQ codes of one recording (the receiver
        side): codes [n_q, 1, F] int64, or packed [1, >= packed bytes] uint8 with n_q and F passed in, as decode_codes takes them.
        want_stages: {"wav", "latents", "cond"}."""
        if n_steps is None or Lw is None or overlap is None:
            raise ValueError("n_steps, Lw and overlap are required")
        noise = self._f32(noise) if noise is not None else None
        pn = noise.data_ptr() if noise is not None else None
        return self._decode_codes_windows(codes, packed, bits, n_q, F, want_stages, lambda cp, pp, st, b, q, f, o, la, co, s:
                                          self.lib.ldc_decode_codes_windows(self._ctx, cp, pp, st, b, q, f, int(t_start), int(n_steps), float(eta),
                                                                            pn, int(Lw), int(overlap), o, la, co, s))

    def decode_codes_dpm_windows(self, codes=None, packed=None, t_start: int = 100, n_steps: int = 10, Lw: Optional[int] = None,
                                 overlap: Optional[int] = None, want_stages: bool = False, bits: int = 10, n_q: Optional[int] = None,
                                 F: Optional[int] = None):
        """`decode_dpm_windows` started from the RVQ codes of one recording; the code arguments as decode_codes_windows."""
        if Lw is None or overlap is None:
            raise ValueError("Lw and overlap are required")
        return self._decode_codes_windows(codes, packed, bits, n_q, F, want_stages, lambda cp, pp, st, b, q, f, o, la, co, s:
                                          self.lib.ldc_decode_codes_dpm_windows(self._ctx, cp, pp, st, b, q, f, int(t_start), int(n_steps),
                                                                                int(Lw), int(overlap), o, la, co, s))

    def unet_forward_items(self, x, t, cond, lens=None):
        """`unet_forward` with a timestep per item (Unet1D.forward's `time[B]`): t a sequence of B timesteps; lens (optional) per-item
        latent lengths as in `unet_forward_ragged`.  eps is zero beyond an item's length."""
        x, cond = self._f32(x), self._f32(cond)
        B, Cx, Lx = x.shape
        ts = self._lengths([int(v) for v in t], B)
        ln = self._lengths(list(lens), B) if lens is not None else None
        eps = self._empty(B, Cx, Lx)
        s = self._enter()
        try:
            L.check(self.lib.ldc_unet_forward_items(self._ctx, x.data_ptr(), ts, cond.data_ptr(), ln, B, Lx, cond.shape[2], eps.data_ptr(), s))
        finally:
            self._exit()
        return eps

    def open_pool(self, slots: int, max_samples: int, sampler: str = "ddpm") -> "DecodePool":
        """A decode pool (ldc_pool_create): `slots` items of up to max_samples samples step together on one captured step graph while each
        keeps its own sampler, timestep, step count, noise and length; items are submitted and popped while the others keep stepping.
        The sampler is a property of an item, not of the pool: `DecodePool.submit(..., t_start=..., eta=...)` admits a DDIM item and
        `DecodePool.submit(..., t_start=..., sampler="dpm")` a DPM-Solver++(2M) item beside DDPM ones.  `sampler` is kept for callers
        that pass "ddpm"; nothing else is a sampler of a pool."""
        if sampler != "ddpm":
            raise ValueError(f"sampler {sampler!r}: a pool has no sampler of its own, every item brings one: "
                             "open the pool without it and pass submit(t_start=..., eta=...) for a DDIM item, "
                             "submit(t_start=..., sampler=\"dpm\") for a DPM-Solver++ item")
        return DecodePool(self, slots, max_samples)

    # ---- the calls a DecodePool makes (a stub engine without a GPU provides these) ------------
    def pool_create(self, slots: int, Lmax: int):
        h = C.c_void_p()
        L.check(self.lib.ldc_pool_create(self._ctx, int(slots), int(Lmax), C.byref(h)))
        return h

    def pool_destroy(self, h) -> None:
        self.lib.ldc_pool_destroy(h)

    def pool_remaining(self, h, slots: int):
        out = (C.c_int32 * slots)()
        L.check(self.lib.ldc_pool_remaining(h, out))
        return list(out)

    def pool_front(self, wav=None, codes=None):
        """the B = 1 front end of one item: -> (start image [1, C, L], raw condition [1, C, F])"""
        if (wav is None) == (codes is None):
            raise ValueError("exactly one of wav / codes")
        cond = self.get_cond(wav) if wav is not None else self.rvq_decode(codes)
        return self.cond_upsample(cond, 2), cond

    def pool_admit(self, h, slot: int, img, cond, n_steps: int, noise=None, seed: int = 0) -> None:
        img, cond = self._f32(img), self._f32(cond)
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        try:
            L.check(self.lib.ldc_pool_admit(self._ctx, h, int(slot), img.data_ptr(), cond.data_ptr(), int(img.shape[-1]), int(n_steps),
                                            noise.data_ptr() if noise is not None else None, int(seed) & (2 ** 64 - 1), s))
        finally:
            self._exit()
        return noise                       # (the tape the library reads: the pool keeps it alive until the item has finished)

    def pool_admit_ddim(self, h, slot: int, img, cond, t_start: int, n_steps: int, eta: float, noise=None, seed: int = 0):
        """ldc_pool_admit_ddim: n_steps DDIM iterations from t_start; noise [n_steps, 1, C, L] or None (Philox with key `seed`)"""
        img, cond = self._f32(img), self._f32(cond)
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        try:
            L.check(self.lib.ldc_pool_admit_ddim(self._ctx, h, int(slot), img.data_ptr(), cond.data_ptr(), int(img.shape[-1]), int(t_start),
                                                 int(n_steps), float(eta), noise.data_ptr() if noise is not None else None,
                                                 int(seed) & (2 ** 64 - 1), s))
        finally:
            self._exit()
        return noise                       # (as pool_admit)

    def pool_admit_dpm(self, h, slot: int, img, cond, t_start: int, n_steps: int) -> None:
        """ldc_pool_admit_dpm: n_steps DPM-Solver++(2M) iterations from t_start; nothing is drawn, so there is no noise and no seed"""
        img, cond = self._f32(img), self._f32(cond)
        s = self._enter()
        try:
            L.check(self.lib.ldc_pool_admit_dpm(self._ctx, h, int(slot), img.data_ptr(), cond.data_ptr(), int(img.shape[-1]), int(t_start),
                                                int(n_steps), s))
        finally:
            self._exit()

    def pool_step(self, h, n: int) -> None:
        s = self._enter()
        try:
            L.check(self.lib.ldc_pool_step(self._ctx, h, int(n), s))
        finally:
            self._exit()

    def pool_take(self, h, slot: int, Lz: int, keep: bool = False):
        """the latents of a finished slot; keep = True leaves the item in its slot (ldc_pool_peek)"""
        lat = self._empty(1, self.main_codec.rep_dims, int(Lz))
        s = self._enter()
        try:
            L.check((self.lib.ldc_pool_peek if keep else self.lib.ldc_pool_take)(self._ctx, h, int(slot), lat.data_ptr(), s))
        finally:
            self._exit()
        return lat

    def pool_evict(self, h, slot: int) -> None:
        L.check(self.lib.ldc_pool_evict(h, int(slot)))

    def pool_back(self, latents):
        """the B = 1 back end of one item: latents [1, C, L] -> waveform [1, 1, L * hop], normalised per item"""
        return self.output_normalise(self.decode_latents(L.MODEL_MAIN, latents), per_item=True)

    def _codes_args(self, codes, packed, bits, n_q, F):
        """-> (codes ptr, packed ptr, packed stride, n_q, B, F, kept tensors) for ldc_decode_codes*"""
        t = self.torch
        if (codes is None) == (packed is None):
            raise ValueError("exactly one of codes / packed")
        if codes is not None:
            codes = codes.to(self.device, t.int64).contiguous()
            n_q, B, F = codes.shape
            return codes.data_ptr(), None, 0, n_q, B, F, codes
        if n_q is None or F is None:
            raise ValueError("a packed payload needs n_q and F")
        packed = packed.to(self.device, t.uint8)
        if packed.dim() != 2 or packed.stride(1) != 1:
            packed = packed.reshape(packed.shape[0], -1).contiguous()
        return None, packed.data_ptr(), packed.stride(0), int(n_q), packed.shape[0], int(F), packed

    def _codes_outputs(self, B, F, want_stages):
        T = F * self.cond_codec.hop_length
        out = self._empty(B, 1, T)
        lat = self._empty(B, self.main_codec.rep_dims, T // self.main_codec.hop_length) if want_stages else None
        cond = self._empty(B, self.main_codec.rep_dims, F) if want_stages else None
        return out, lat, cond

    def decode_codes(self, codes=None, packed=None, bits: int = 10, n_steps: Optional[int] = None, noise=None, per_item: bool = False,
                     want_stages: bool = False, n_q: Optional[int] = None, F: Optional[int] = None):
        """`decode` started from RVQ codes (the receiver side): codes [n_q, B, F] int64, or packed [B, >= packed bytes] uint8 (the
        BitPacker payload of `bits` per code; n_q and F passed in).  want_stages: {"wav", "latents", "cond"}."""
        if n_steps is None:
            raise ValueError("n_steps is required")
        cp, pp, stride, n_q, B, F, keep = self._codes_args(codes, packed, bits, n_q, F)
        out, lat, cond = self._codes_outputs(B, F, want_stages)
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        p = lambda t: t.data_ptr() if t is not None else None
        L.check(self.lib.ldc_decode_codes(self._ctx, cp, pp, stride, int(bits), n_q, B, F, int(n_steps), p(noise), int(per_item),
                                          out.data_ptr(), p(lat), p(cond), s))
        self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond}
        return out

    def decode_codes_ddim(self, codes=None, packed=None, bits: int = 10, t_start: int = 100, n_steps: int = 10, eta: float = 0.0,
                          noise=None, per_item: bool = False, want_stages: bool = False, n_q: Optional[int] = None,
                          F: Optional[int] = None):
        """`decode_ddim` started from RVQ codes; the code arguments as decode_codes."""
        cp, pp, stride, n_q, B, F, keep = self._codes_args(codes, packed, bits, n_q, F)
        out, lat, cond = self._codes_outputs(B, F, want_stages)
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        p = lambda t: t.data_ptr() if t is not None else None
        L.check(self.lib.ldc_decode_codes_ddim(self._ctx, cp, pp, stride, int(bits), n_q, B, F, int(t_start), int(n_steps), float(eta),
                                               p(noise), int(per_item), out.data_ptr(), p(lat), p(cond), s))
        self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond}
        return out

    def decode_codes_dpm(self, codes=None, packed=None, bits: int = 10, t_start: int = 100, n_steps: int = 10, per_item: bool = False,
                         want_stages: bool = False, n_q: Optional[int] = None, F: Optional[int] = None):
        """`decode_dpm` started from RVQ codes; the code arguments as decode_codes."""
        cp, pp, stride, n_q, B, F, keep = self._codes_args(codes, packed, bits, n_q, F)
        out, lat, cond = self._codes_outputs(B, F, want_stages)
        s = self._enter()
        p = lambda t: t.data_ptr() if t is not None else None
        try:
            L.check(self.lib.ldc_decode_codes_dpm(self._ctx, cp, pp, stride, int(bits), n_q, B, F, int(t_start), int(n_steps), int(per_item),
                                                  out.data_ptr(), p(lat), p(cond), s))
        finally:
            self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond}
        return out

    def decode_codes_ragged(self, codes=None, packed=None, frames=None, bits: int = 10, n_steps: Optional[int] = None, t_start: int = 0,
                            eta: float = 0.0, noise=None, want_stages: bool = False, n_q: Optional[int] = None, F: Optional[int] = None):
        """`decode_codes` (t_start 0) / `decode_codes_ddim` (t_start > 0) of items of different lengths in one call: frames[b] condition
        frames of item b are its own (multiples of chunk_quantum // 320).  codes [n_q, B, Fmax] int64, or packed [B, stride] uint8 whose
        row b holds item b's own payload of packed_bytes(n_q, frames[b], bits) bytes (n_q passed in; Fmax = F or max(frames)); what
        lies behind an item's frames / bytes is never read.  Every item comes out as if decoded alone; outputs are zero beyond an
        item's length.  want_stages: {"wav", "latents", "cond"}."""
        if n_steps is None:
            raise ValueError("n_steps is required")
        if frames is None:
            raise ValueError("frames is required")
        frames = [int(v) for v in frames]
        if packed is not None and F is None:
            F = max(frames)
        cp, pp, stride, n_q, B, F, keep = self._codes_args(codes, packed, bits, n_q, F)
        fr = self._lengths(frames, B)
        out, lat, cond = self._codes_outputs(B, F, want_stages)
        noise = self._f32(noise) if noise is not None else None
        s = self._enter()
        p = lambda t: t.data_ptr() if t is not None else None
        try:
            L.check(self.lib.ldc_decode_codes_ragged(self._ctx, cp, pp, stride, int(bits), n_q, B, F, fr, int(t_start), int(n_steps),
                                                     float(eta), p(noise), out.data_ptr(), p(lat), p(cond), s))
        finally:
            self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond}
        return out

    # ---- item seeds: every item of a batch draws its noise as if alone ----------
    SEEDED_SAMPLERS = {"ddpm": 0, "ddim": 1}

    @staticmethod
    def _seeds(seeds, B: int):
        if seeds is None:
            return None   # (the library refuses, with the value named)
        seeds = [int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds]
        if len(seeds) != B:
            raise ValueError(f"{len(seeds)} seeds for a batch of {B}")
        return (C.c_uint64 * B)(*seeds)

    def _seeded_sampler(self, sampler):
        return self.SEEDED_SAMPLERS.get(sampler, sampler) if isinstance(sampler, str) else int(sampler)

    def sample_seeded(self, img, cond, seeds, n_steps: int, sampler="ddpm", t_start: int = 0, eta: float = 0.0):
        """`denoise` (sampler "ddpm") / `ddim_sample` (sampler "ddim", from t_start) on the start image `img` with one seed per item:
        item b draws what `reseed(seeds[b])` followed by the same call at B = 1 on the item alone draws, wherever it sits in the
        batch.  The engine's noise epoch is neither read nor advanced."""
        img = self._f32(img).clone()
        cond = self._f32(cond)
        B, _, Lx = img.shape
        sd = self._seeds(seeds, B)
        s = self._enter()
        try:
            L.check(self.lib.ldc_sample_seeded(self._ctx, img.data_ptr(), cond.data_ptr(), self._seeded_sampler(sampler), int(t_start),
                                               int(n_steps), float(eta), sd, B, Lx, cond.shape[2], s))
        finally:
            self._exit()
        return img

    def decode_seeded(self, wav, seeds, n_steps: int, lengths=None, sampler="ddpm", t_start: int = 0, eta: float = 0.0,
                      want_stages: bool = False):
        """`decode` / `decode_ddim` (lengths None) or `decode_ragged` (lengths[b] samples of item b) with one seed per item and
        per-item normalisation at both ends: item b comes out as `reseed(seeds[b])` followed by the decode of the item alone gives
        it, whatever the batch size, the packing and the item's position."""
        wav = self._f32(wav)
        B, _, T = wav.shape
        F, Lz = T // self.cond_codec.hop_length, T // self.main_codec.hop_length
        lens = self._lengths(list(lengths), B) if lengths is not None else None
        sd = self._seeds(seeds, B)
        out = self._empty(B, 1, T)
        lat = self._empty(B, self.main_codec.rep_dims, Lz) if want_stages else None
        cond = self._empty(B, self.main_codec.rep_dims, F) if want_stages else None
        n_q = self.cond_codec.n_q_for_bandwidth(None)
        codes = self._empty(n_q, B, F, dtype=self.torch.int64) if want_stages else None
        s = self._enter()
        p = lambda t: t.data_ptr() if t is not None else None
        try:
            L.check(self.lib.ldc_decode_seeded(self._ctx, wav.data_ptr(), lens, B, T, self._seeded_sampler(sampler), int(t_start), int(n_steps),
                                               float(eta), sd, out.data_ptr(), p(lat), p(cond), p(codes), s))
        finally:
            self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond, "codes": codes}
        return out

    def decode_codes_seeded(self, seeds, codes=None, packed=None, lengths=None, bits: int = 10, n_steps: Optional[int] = None,
                            sampler="ddpm", t_start: int = 0, eta: float = 0.0, want_stages: bool = False, n_q: Optional[int] = None,
                            F: Optional[int] = None):
        """`decode_codes` / `decode_codes_ddim` (lengths None) or `decode_codes_ragged` (lengths[b] condition frames of item b) with one
        seed per item and per-item normalisation: the contract of `decode_seeded`; the code arguments as decode_codes_ragged."""
        if n_steps is None:
            raise ValueError("n_steps is required")
        frames = [int(v) for v in lengths] if lengths is not None else None
        if packed is not None and F is None and frames is not None:
            F = max(frames)
        cp, pp, stride, n_q, B, F, keep = self._codes_args(codes, packed, bits, n_q, F)
        fr = self._lengths(frames, B) if frames is not None else None
        sd = self._seeds(seeds, B)
        out, lat, cond = self._codes_outputs(B, F, want_stages)
        s = self._enter()
        p = lambda t: t.data_ptr() if t is not None else None
        try:
            L.check(self.lib.ldc_decode_codes_seeded(self._ctx, cp, pp, stride, int(bits), n_q, B, F, fr, self._seeded_sampler(sampler),
                                                     int(t_start), int(n_steps), float(eta), sd, out.data_ptr(), p(lat), p(cond), s))
        finally:
            self._exit()
        if want_stages:
            return {"wav": out, "latents": lat, "cond": cond}
        return out

    # ---- accounting ------------------------------------------------------------------------------
    def unet_step_cost(self, B: int, Lz: int):
        fl, by = C.c_double(), C.c_double()
        L.check(self.lib.ldc_unet_step_cost(self._ctx, B, Lz, C.byref(fl), C.byref(by)))
        return fl.value, by.value

    def timeline(self, n_steps: int, parts: int = 2):
        """Device-side timeline of the last sampler call (after timeline_enable(True)): per batch part an array
        [n_steps, 2] of begin / end times in microseconds relative to the earliest stamp."""
        out = []
        for k in range(parts):
            buf = (C.c_uint64 * (2 * n_steps))()
            L.check(self.lib.ldc_timeline_read(self._ctx, k, n_steps, buf))
            out.append(np.array(buf, dtype=np.float64).reshape(n_steps, 2))
        t0 = min(float(a[a > 0].min()) for a in out if (a > 0).any())
        return [(a - t0) / 100.0 for a in out]      # 100 MHz ticks -> us

    def kstamps_enable(self, on: bool):
        L.check(self.lib.ldc_kstamps_enable(self._ctx, int(on)))

    def kstamps_reset(self):
        L.check(self.lib.ldc_kstamps_reset(self._ctx))

    def kstamps(self, part: int, n_steps: int):
        """Timed-mode stamps of batch part `part` after a decode with kstamps_enable(True): (ticks [n_steps, n_ops, 2] in
        microseconds on the device's 100 MHz clock (0 where the op is not a pipelined conv), op descriptions, class codes)."""
        n = C.c_int()
        L.check(self.lib.ldc_kstamps_read(self._ctx, part, n_steps, C.byref(n), None, None, 0, None))
        nops, cap = n.value, 96
        ticks = (C.c_uint64 * (n_steps * nops * 2))()
        infos = C.create_string_buffer(nops * cap)
        classes = (C.c_int * nops)()
        L.check(self.lib.ldc_kstamps_read(self._ctx, part, n_steps, C.byref(n), ticks, infos, cap, classes))
        t = np.array(ticks, dtype=np.float64).reshape(n_steps, nops, 2) / 100.0
        names = [infos.raw[o * cap:(o + 1) * cap].split(b"\0", 1)[0].decode() for o in range(nops)]
        return t, names, list(classes)

    def timeline_enable(self, on: bool):
        L.check(self.lib.ldc_timeline_enable(self._ctx, int(on)))

    def profile(self, on: bool):
        L.check(self.lib.ldc_profile_enable(self._ctx, int(on)))

    def profile_read(self):
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        L.check(self.lib.ldc_profile_read(self._ctx, C.byref(ms), C.byref(n), C.byref(fl)))
        return ms.value, n.value, fl.value

    CLASS_NAMES = ("other", "conv_gemm", "gn_apply", "layernorm", "linear_attention", "attention_full", "elementwise")

    def profile_read_classes(self):
        """Per kernel class: (name, ms, launches, algorithmic flops, algorithmic bytes) of the profiling pass."""
        n = len(self.CLASS_NAMES)
        ms, la, fl, by = (C.c_double * n)(), (C.c_int64 * n)(), (C.c_double * n)(), (C.c_double * n)()
        L.check(self.lib.ldc_profile_read_classes(self._ctx, n, ms, la, fl, by))
        return [(self.CLASS_NAMES[k], ms[k], la[k], fl[k], by[k]) for k in range(n)]

    # ---- L1 primitives (parity tests) ------------------------------------------------------------
    def sconv1d(self, x, w, b, stride=1, dilation=1, causal=True, pre_elu=False):
        x = self._f32(x)
        w = np.ascontiguousarray(w, np.float32); b = np.ascontiguousarray(b, np.float32)
        B, Cin, Lx = x.shape
        Cout, _, k = w.shape
        Lout = -(-Lx // stride)
        y = self._empty(B, Cout, Lout)
        s = self._enter()
        L.check(self.lib.ldc_sconv1d(self._ctx, x.data_ptr(), B, Cin, Lx, w.ctypes.data_as(C.c_void_p),
                                     b.ctypes.data_as(C.c_void_p), Cout, k, stride, dilation, int(causal), int(pre_elu),
                                     y.data_ptr(), s))
        self._exit()
        return y

    def sconvtr1d(self, x, w, b, stride, causal):
        x = self._f32(x)
        w = np.ascontiguousarray(w, np.float32); b = np.ascontiguousarray(b, np.float32)
        B, Cin, Lx = x.shape
        _, Cout, k = w.shape
        y = self._empty(B, Cout, Lx * stride)
        s = self._enter()
        L.check(self.lib.ldc_sconvtr1d(self._ctx, x.data_ptr(), B, Cin, Lx, w.ctypes.data_as(C.c_void_p),
                                       b.ctypes.data_as(C.c_void_p), Cout, k, stride, int(causal), y.data_ptr(), s))
        self._exit()
        return y

    def slstm(self, x, weights: Sequence[np.ndarray], layers: int):
        x = self._f32(x)
        B, H, T = x.shape
        ws = [np.ascontiguousarray(w, np.float32) for w in weights]
        arr = (C.c_void_p * len(ws))(*[w.ctypes.data_as(C.c_void_p) for w in ws])
        y = self._empty(B, H, T)
        s = self._enter()
        L.check(self.lib.ldc_slstm(self._ctx, x.data_ptr(), B, H, T, arr, layers, y.data_ptr(), s))
        self._exit()
        return y


# --------------------------------------------------------------------------------------------------
# reference-shaped facade
# --------------------------------------------------------------------------------------------------
class CodecStream:
    """B independent streams through the encoder (side = lib.STREAM_ENCODER) or decoder (lib.STREAM_DECODER) of one codec; the state a
    chunk needs from the past -- conv context rows, transposed-conv rows, LSTM (h, c) -- lives on the device (Engine.open_stream)."""

    def __init__(self, eng: Engine, which: int, side: int, B: int):
        self.eng, self.which, self.side, self.B = eng, int(which), int(side), int(B)
        self._st = C.c_void_p()
        L.check(eng.lib.ldc_stream_create(eng._ctx, self.which, self.side, self.B, C.byref(self._st)))
        eng._streams.append(self)           # (Engine.close destroys the sessions it still has before the context)
        self.hop = (eng.cond_codec if which == L.MODEL_COND else eng.main_codec).hop_length
        self.min_first = L.stream_min_first(eng._cfg, self.which, self.side)

    def _call(self, fn, *args):
        s = self.eng._enter()
        try:
            L.check(fn(self.eng._ctx, self._st, *args, s))
        finally:
            self.eng._exit()

    def encode(self, wav):
        """wav [B, 1, T], T a multiple of the hop -> z [B, D, T / hop]"""
        e = self.eng
        wav = e._f32(wav)
        T = wav.shape[-1]
        z = e._empty(self.B, e.main_codec.rep_dims, max(0, T // self.hop))
        self._call(e.lib.ldc_seanet_encode_stream, wav.data_ptr(), int(T), z.data_ptr())
        return z

    def decode(self, z):
        """z [B, D, L] -> wav [B, 1, L * hop]"""
        e = self.eng
        z = e._f32(z)
        Lz = z.shape[-1]
        wav = e._empty(self.B, 1, max(0, Lz * self.hop))
        self._call(e.lib.ldc_seanet_decode_stream, z.data_ptr(), int(Lz), wav.data_ptr())
        return wav

    def get_cond(self, wav, bandwidth: Optional[float] = None, return_codes: bool = False):
        """the cond encoder's stream: wav [B, 1, T] -> cond [B, D, T / 320] (and codes [n_q, B, T / 320])"""
        e = self.eng
        wav = e._f32(wav)
        T = wav.shape[-1]
        F = max(0, T // self.hop)
        bw = float(bandwidth) if bandwidth else 0.0
        n_q = e.cond_codec.n_q_for_bandwidth(bw if bw > 0 else None) if e.cond_codec is not None else 1
        cond = e._empty(self.B, e.main_codec.rep_dims, F)
        codes = e._empty(n_q, self.B, F, dtype=e.torch.int64) if return_codes else None
        self._call(e.lib.ldc_get_cond_stream, wav.data_ptr(), int(T), bw, cond.data_ptr(), codes.data_ptr() if codes is not None else None)
        return (cond, codes) if return_codes else cond

    def reset(self, mask=None):
        """make the items with mask[b] true (all when mask is None) fresh: their next chunk starts a sequence"""
        m = None
        if mask is not None:
            m = (C.c_uint8 * self.B)(*[1 if bool(v) else 0 for v in mask])
        s = self.eng._enter()
        try:
            L.check(self.eng.lib.ldc_stream_reset(self._st, m, s))
        finally:
            self.eng._exit()

    def close(self):
        if getattr(self, "_st", None) is not None and self._st:
            self.eng.lib.ldc_stream_destroy(self._st)
            self._st = None
            if self in self.eng._streams:
                self.eng._streams.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DecodePool:
    """A fixed set of slots that step together (Engine.open_pool, ldc_pool_*): `submit` admits an item into a free slot, `step`
    advances every running item, `finished` lists the tickets whose items are done, `pop` takes one out and decodes its waveform.
    An item comes out as `Engine.denoise` (a DDPM item), `Engine.ddim_sample` (a DDIM item, `submit(t_start=...)`) or
    `Engine.dpm_sample` (a DPM-Solver++(2M) item, `submit(t_start=..., sampler="dpm")`) gives it alone
    at B = 1, whatever the other slots hold -- any sampler, any schedule -- within rounding.  The bookkeeping
    here is plain Python over the library's host mirror (`pool_remaining`); the engine may be any object with the `pool_*` methods."""

    def __init__(self, eng, slots: int, max_samples: int):
        self.eng, self.slots = eng, int(slots)
        hop = eng.main_codec.hop_length
        if max_samples <= 0 or max_samples % hop:
            raise ValueError(f"max_samples {max_samples} must be a positive multiple of the hop {hop}")
        self.hop, self.Lmax = hop, int(max_samples) // hop
        self._h = eng.pool_create(self.slots, self.Lmax)
        if hasattr(eng, "_pools"):
            eng._pools.append(self)         # (Engine.close destroys the pools it still has before the context)
        self._slot_of = {}                  # ticket -> slot
        self._info = {}                     # ticket -> (latent length, noise tape kept alive)
        self._next = 0

    def remaining(self):
        """per slot: -1 free, 0 finished, k > 0 steps to go"""
        return self.eng.pool_remaining(self._h, self.slots)

    def free_slots(self):
        return [i for i, r in enumerate(self.remaining()) if r < 0]

    def submit(self, wav=None, codes=None, n_steps: int = 50, noise=None, seed=None, t_start: int = 0, eta: float = 0.0,
               sampler: Optional[str] = None) -> int:
        """wav [1, 1, T] or codes [n_q, 1, F] of ONE item; noise [n_steps, 1, C, L] or None (Philox with key `seed`, the ticket number when
        None).  sampler None: t_start 0 (the convention of `Engine.decode_ragged`) is halfway DDPM sampling, n_steps steps; t_start > 0 is
        n_steps DDIM iterations from t_start with `eta`, and `remaining` counts iterations.  sampler "dpm": n_steps DPM-Solver++(2M)
        iterations from t_start >= 1; nothing is drawn, so a `noise`, a `seed` or a non-zero `eta` is a ValueError.  "ddpm" (t_start 0)
        and "ddim" (t_start >= 1) name the two routes of None.  -> ticket.  Raises when no slot is free."""
        if sampler not in (None, "ddpm", "ddim", "dpm"):
            raise ValueError(f"sampler {sampler!r}: an item's sampler is \"ddpm\", \"ddim\" or \"dpm\" (None: by t_start)")
        if sampler == "dpm":
            given = [n for n, bad in (("noise", noise is not None), ("seed", seed is not None), ("eta", float(eta) != 0.0)) if bad]
            if given:
                raise ValueError(f"sampler \"dpm\" draws nothing: {', '.join(given)} would be ignored, leave it out")
        if sampler in ("ddim", "dpm") and int(t_start) < 1:
            raise ValueError(f"sampler {sampler!r} needs t_start >= 1, not {t_start}")
        if sampler == "ddpm" and t_start:
            raise ValueError(f"sampler \"ddpm\" runs n_steps steps from t = n_steps - 1: t_start = {t_start} must be 0")
        free = self.free_slots()
        if not free:
            raise RuntimeError(f"no free slot in a pool of {self.slots}: step until an item has finished and pop it")
        img, cond = self.eng.pool_front(wav=wav, codes=codes)
        ticket = self._next
        key = ticket if seed is None else int(seed)
        if sampler == "dpm":
            kept = self.eng.pool_admit_dpm(self._h, free[0], img, cond, int(t_start), int(n_steps))
        elif t_start:
            kept = self.eng.pool_admit_ddim(self._h, free[0], img, cond, int(t_start), int(n_steps), float(eta), noise, key)
        else:
            kept = self.eng.pool_admit(self._h, free[0], img, cond, int(n_steps), noise, key)
        self._next += 1
        self._slot_of[ticket] = free[0]
        self._info[ticket] = (int(img.shape[-1]), kept)
        return ticket

    def step(self, n: int = 1) -> None:
        self.eng.pool_step(self._h, int(n))

    def finished(self):
        """tickets whose items are done, in submission order"""
        rem = self.remaining()
        return [t for t in sorted(self._slot_of) if rem[self._slot_of[t]] == 0]

    def running(self):
        rem = self.remaining()
        return [t for t in sorted(self._slot_of) if rem[self._slot_of[t]] > 0]

    def pop(self, ticket: int):
        """-> {"wav" [1, 1, T], "latents" [1, C, L]} of a finished item; its slot is free again"""
        if ticket not in self._slot_of:
            raise KeyError(f"ticket {ticket} is not in the pool")
        slot = self._slot_of[ticket]
        lat = self.eng.pool_take(self._h, slot, self._info[ticket][0])
        del self._slot_of[ticket], self._info[ticket]
        return {"wav": self.eng.pool_back(lat), "latents": lat}

    def peek(self, ticket: int):
        """the latents [1, C, L] of a finished item that stays in its slot"""
        return self.eng.pool_take(self._h, self._slot_of[ticket], self._info[ticket][0], keep=True)

    def evict(self, ticket: int) -> None:
        slot = self._slot_of.pop(ticket)
        del self._info[ticket]
        self.eng.pool_evict(self._h, slot)

    def run_until_done(self) -> None:
        while True:
            rem = [r for r in self.remaining() if r > 0]
            if not rem:
                return
            self.step(min(rem))             # (to the next item that finishes: nothing idles longer than it must)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            self.eng.pool_destroy(self._h)
            self._h = None
            if self in getattr(self.eng, "_pools", []):
                self.eng._pools.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Upsampler:
    """Stands for `diff_model.upsampling_layers`: iterating yields one callable that applies the WHOLE
    stack (the reference applies them in sequence, sample.py:127-128), so `for layer in
    model.diff_model.upsampling_layers: img = layer(img)` gives the same tensor."""

    def __init__(self, eng: Engine):
        self._eng = eng

    def __iter__(self):
        yield lambda img: self._eng.cond_upsample(img, 0)

    def __len__(self):
        return 1


class _DiffModel:
    def __init__(self, eng: Engine):
        self._eng = eng
        self.upsampling_layers = _Upsampler(eng)
        self.channels = eng.unet.inp_channels
        self.self_condition = False

    def __call__(self, x, time, x_cond=None):
        t = int(time.reshape(-1)[0].item()) if hasattr(time, "reshape") else int(time)
        if hasattr(time, "reshape") and bool((time != t).any()):      # a timestep per item (unet.py:422-437): the per-item plan
            return self._eng.unet_forward_items(x, [int(v) for v in time.reshape(-1).tolist()], x_cond)
        return self._eng.unet_forward(x, t, x_cond)


class _Diffusion:
    def __init__(self, eng: Engine):
        self._eng = eng
        self.seq_length = None
        self.num_timesteps = eng.unet.timesteps
        # ddpm_loss.py:125-132 (is_ddim_sampling is hard-coded False there; set it to sample with DDIM)
        self.sampling_timesteps = eng.unet.timesteps
        self.ddim_sampling_eta = 0.0
        self.is_ddim_sampling = False

    def p_sample(self, x, t: int, condition=None, noise=None):
        return self._eng.p_sample(x, t, condition, noise), None

    def halfway_sampling(self, img=None, t=None, condition=None, noise=None):
        if tuple(img.shape) == tuple(condition.shape):       # ddpm_loss.py:376-378
            if self._eng.unet.upsampling_ratios is None:
                # the reference iterates model.upsampling_layers here, an attribute that does not exist without
                # upsampling_ratios (unet.py:372): same error, same place
                raise AttributeError("'Unet1D' object has no attribute 'upsampling_layers'")
            img = self._eng.cond_upsample(img, 0)
        return self._eng.denoise(img, condition, int(t), noise)

    def p_sample_loop(self, shape, condition=None, img=None, noise=None):
        """ddpm_loss.py:253-266; `img`/`noise` inject the start image and the per-step draws (parity runs)."""
        return self._eng.p_sample_loop(condition, img=img, noise=noise, length=shape[2])

    def ddim_sample(self, shape, condition=None, clip_denoised=True, img=None, noise=None):
        """ddpm_loss.py:268-303: sampling_timesteps DDIM iterations from num_timesteps with eta = ddim_sampling_eta;
        `img`/`noise` inject the start image and the [S, B, C, L] draws (parity runs)."""
        if not clip_denoised:
            raise NotImplementedError("ddim_sample runs with clip_denoised=True only")
        return self._eng.ddim_sample(condition, int(self.num_timesteps), int(self.sampling_timesteps), float(self.ddim_sampling_eta),
                                     img=img, noise=noise, length=shape[2])

    def sample(self, batch_size=16, condition=None):
        """ddpm_loss.py:305-309: p_sample_loop, or ddim_sample when is_ddim_sampling is set."""
        assert self.seq_length is not None, "set diffusion.seq_length as the reference's constructor does"
        fn = self.ddim_sample if self.is_ddim_sampling else self.p_sample_loop
        return fn((batch_size, self._eng.unet.inp_channels, self.seq_length), condition)

    def infilling(self, infill_img, condition, midway_t=None, noise=None, offset=0, lam=0.8, img=None, noises=None):
        """ddpm_loss.py:331-367 (`noise` and `offset` are accepted and unused, as in the reference); `img`/`noises`
        inject the start image and the 2*midway_t draws (parity runs)."""
        out, _ = self._eng.infilling(infill_img, condition, int(midway_t), lam=lam, img=img, noise=noises)
        return out


class DiffAudioRep:
    """Facade with the reference's attribute names over one side (main or cond) of an Engine."""

    def __init__(self, eng: Engine, which: int):
        self._eng, self._which = eng, which
        cfg = eng.cond_codec if which == L.MODEL_COND else eng.main_codec
        self.frame_rate = cfg.frame_rate
        self.bandwidth = cfg.bandwidth
        self.quantization = cfg.quantization
        if which == L.MODEL_MAIN:
            self.diff_model = _DiffModel(eng)
            self.diffusion = _Diffusion(eng)

    def eval(self):
        return self

    def to(self, *_a, **_k):
        return self

    def encoder(self, wav):
        return self._eng.encode(self._which, wav)

    def decoder(self, z):
        return self._eng.decode_latents(self._which, z)

    def quantizer(self, x, sample_rate=None, bandwidth=None, n_q=None):
        cfg = self._eng.cond_codec
        n = n_q if n_q is not None else cfg.n_q_for_bandwidth(bandwidth)
        q, codes = self._eng.rvq(x, n)
        torch = self._eng.torch
        bw = torch.tensor(n * 0.5).to(q)
        return QuantizedResult(q, codes, bw, penalty=torch.zeros((), device=q.device))

    def get_cond(self, x):
        if self._which != L.MODEL_COND:
            return self.encoder(x)
        return self._eng.get_cond(x)
