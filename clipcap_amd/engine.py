"""Device-side engines: flat parameter arenas + workspaces + calls into libclipcap_hip.so.

``MapperEngine`` / ``Gpt2Engine`` own the arenas the C ABI works on (fp32 master ``w32``, bf16 operand copy ``w16``,
fp32 gradient arena ``g32``) and hand out named views with the reference's state-dict names and layouts
(clipcap/model/mapper.py, clipcap/model/attention.py; HF GPT-2 names).  ``ClipCapEngine`` chains them into the
training step of clipcap/model/model.py:94-113 (forward + backward, no autograd graph).

PyTorch is used for device memory and streams only; all arithmetic runs in the HIP library.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import torch

from clipcap_amd import _lib
from clipcap_amd._lib import OP_BF16, OP_FP16, OP_X3, Gpt2Cfg, Gpt2Shape, MapperCfg, check, op_dtype_of


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_cuda(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: clipcap_amd runs on an MI355X only (tensor is on {t.device}); there is no CPU fallback")


MAPPER_LAYER_NAMES = ["norm1.weight", "norm1.bias", "attn.to_queries.weight", "attn.to_keys_values.weight", "attn.project.weight",
                      "attn.project.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                      "mlp.fc2.bias"]
GPT2_LAYER_NAMES = ["ln_1.weight", "ln_1.bias", "attn.c_attn.weight", "attn.c_attn.bias", "attn.c_proj.weight", "attn.c_proj.bias",
                    "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias"]


class _Arena:
    """fp32 master + bf16 operand copy (+ lazily a gradient arena and AdamW state) for one parameter family."""

    def __init__(self, n: int, device, sync_fn=None, op_dtype: int = OP_BF16):
        self.n = n
        self.device = torch.device(device)
        self.sync_fn = sync_fn   # (w32_ptr or None, w16_ptr, stream) -> rc : cast + transposed GEMM-weight copies (None: transposed copies only)
        self.op_dtype = op_dtype
        self.w32 = torch.zeros(n, dtype=torch.float32, device=self.device)
        # [0,n): 16-bit cast of the master (bf16 or fp16, cfg.op_dtype); [n,2n): transposed copies of the GEMM weights
        # (include/clipcap_hip.h Conventions).  bf16x3: 6n elements — [hi | lo | hi] row images of every GEMM weight and of its transpose
        self.w16 = self._alloc_w16() if self.device.type == "cuda" else None
        self.g32: Optional[torch.Tensor] = None
        self.m: Optional[torch.Tensor] = None
        self.v: Optional[torch.Tensor] = None
        # exponential moving average of the master (enable_ema / adamw_step(ema_decay=...)); None: no average is kept.  Like m / v it
        # covers the own range only once the optimizer state is sharded
        self.ema: Optional[torch.Tensor] = None
        self._w16_version = -1
        # optimizer-state sharding (train/ddp.py ZeroShard): (rank, [(lo, hi)] per rank, gather(t, ranges)).  m / v then cover the own range only
        self.zero = None
        # tensors aliasing w32 whose in-place writes do NOT bump w32._version: nn.Parameters re-pointed with ``p.data = view``
        # (ArenaModule._rebind) carry their own version counters, so load_state_dict / torch optimizers writing through them
        # would otherwise leave the bf16 operand copy stale.  The dirty stamp is the sum over w32 and every watched alias.
        self.watch: List[torch.Tensor] = []

    def _alloc_w16(self) -> torch.Tensor:
        return torch.zeros((6 if self.op_dtype == OP_X3 else 2) * self.n, dtype=torch.float16 if self.op_dtype == OP_FP16 else torch.bfloat16,
                           device=self.device)

    def mark_dirty(self) -> None:
        """The fp32 master was written behind torch's back (a raw-pointer writer: an RCCL broadcast into the arena, a C-ABI caller):
        the operand copy is rebuilt before its next use."""
        self._w16_version = -1

    def _stamp(self) -> int:
        s = self.w32._version
        for t in self.watch:
            s += t._version
        return s

    def sync_bf16(self):
        """Refresh the bf16 copy if the master changed (through w32, one of its views, or a watched parameter alias)."""
        if self._stamp() != self._w16_version:
            self.refresh_bf16()

    def refresh_bf16(self):
        check(self.sync_fn(_p(self.w32), _p(self.w16), _stream(self.device)), "cc_*_sync_weights")
        self._w16_version = self._stamp()

    def set_op_dtype(self, op_dtype: int) -> None:
        """Switch the operand copy between bf16, fp16 and the split-bf16 images (rebuilt lazily from the fp32 master)."""
        if op_dtype != self.op_dtype:
            self.op_dtype = op_dtype
            if self.w16 is not None:
                self.w16 = self._alloc_w16()
            self._w16_version = -1

    def moved_to(self, device, sync_fn) -> "_Arena":
        """A copy of this arena on `device` carrying the master, the gradient arena, the AdamW moments and the weight average (resume()
        followed by .to(device) must not lose the optimizer state)."""
        new = _Arena(self.n, device, sync_fn, self.op_dtype)
        new.w32.copy_(self.w32)
        for name in ("g32", "m", "v", "ema"):
            t = getattr(self, name)
            if t is not None:
                setattr(new, name, t.to(new.device))
        return new

    def shard_optimizer_state(self, rank: int, world: int, gather) -> None:
        """ZeRO stage 1 (the reference's --deepspeed-strategy, clipcap/train/args.py:87-92, which Lightning hands to DeepSpeed): this rank
        keeps the AdamW moments of elements [lo, hi) of the arena only and steps only those; ``gather(w32, ranges)`` then broadcasts every
        owner's updated slice (ddp.ZeroShard).  Gradients stay all-reduced over the whole arena, so the update of an element is the one
        the unsharded step computes, bit for bit.  Full moments already present (a resumed run) are cut down to the own range, and so is
        a full weight average."""
        per = (((self.n + world - 1) // world) + 7) // 8 * 8
        ranges = [(min(self.n, r * per), min(self.n, (r + 1) * per)) for r in range(world)]
        lo, hi = ranges[rank]
        for name in ("m", "v", "ema"):
            t = getattr(self, name)
            if t is not None and t.numel() == self.n:
                setattr(self, name, t[lo:hi].clone())
        self.zero = (rank, ranges, gather)

    def full_moments(self):
        """(m, v) over the whole arena.  Replicated state: the device tensors themselves.  Sharded state (ZeRO stage 1): a COLLECTIVE (every
        rank calls it) that moves one owner's slice at a time through a slice-sized device buffer into HOST tensors — peak device memory is
        one slice, not two more full-size arenas on every rank (which is what sharding was meant to save)."""
        if self.zero is None or self.m is None:
            return self.m, self.v
        return self._full_host(self.m), self._full_host(self.v)

    def _full_host(self, t: torch.Tensor) -> torch.Tensor:
        """Sharded state ``t`` (own range) over the whole arena as a HOST tensor, one owner's slice at a time (a collective)."""
        rank, ranges, gather = self.zero
        full = torch.empty(self.n, dtype=torch.float32)                  # host
        for r, (a, b) in enumerate(ranges):
            if b <= a:
                continue
            piece = t if r == rank else torch.empty(b - a, dtype=torch.float32, device=self.device)
            gather(piece, [(0, b - a) if q == r else (0, 0) for q in range(len(ranges))])     # one broadcast: owner r's slice
            full[a:b].copy_(piece)
            del piece
        return full

    def enable_ema(self) -> None:
        """Start the weight average at the current master: ema_0 = p_0.  With sharded optimizer state: the own range only.  A no-op if
        an average is already kept."""
        if self.ema is not None:
            return
        if self.zero is not None:
            lo, hi = self.zero[1][self.zero[0]]
            self.ema = self.w32[lo:hi].clone()
        else:
            self.ema = self.w32.clone()

    def full_ema(self) -> Optional[torch.Tensor]:
        """The weight average over the whole arena.  Replicated state: the device tensor itself.  Sharded state: a COLLECTIVE like
        full_moments, returning a HOST tensor filled one owner's slice at a time."""
        if self.zero is None or self.ema is None:
            return self.ema
        return self._full_host(self.ema)

    def ema_on_device(self) -> Optional[torch.Tensor]:
        """The weight average over the whole arena on the device.  Sharded state: a COLLECTIVE — a full-size buffer, the own slice copied
        in, the owners' slices exchanged as the parameters are after a step."""
        if self.zero is None or self.ema is None:
            return self.ema
        rank, ranges, gather = self.zero
        lo, hi = ranges[rank]
        buf = torch.empty(self.n, dtype=torch.float32, device=self.device)
        buf[lo:hi].copy_(self.ema)
        gather(buf, ranges)
        return buf

    def grads(self) -> torch.Tensor:
        if self.g32 is None:
            self.g32 = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        return self.g32

    def _adamw(self, p, g, m, v, n, w16, lr, step, betas, eps, weight_decay, grad_scale, scaler, clip, ema_decay=None) -> None:
        """One AdamW launch over n elements; w16 None: no cast.  ``clip`` None: the entry points every step used before clipping existed.
        ``ema_decay`` given: cc_adamw_step_ema (clip nullable), which also averages self.ema — the n elements matching p."""
        l, st = _lib.lib(), _stream(self.device)
        step = 0 if scaler is not None else step      # with a loss scaler the step number is its device-side count of applied steps
        ls = _p(scaler.scale) if scaler is not None else None
        fi = _p(scaler.found_inf) if scaler is not None else None
        if ema_decay is not None:
            assert self.ema.numel() == n
            check(l.cc_adamw_step_ema(self.op_dtype, _p(p), _p(g), _p(m), _p(v), n, lr, betas[0], betas[1], eps, weight_decay, step, grad_scale,
                                      ls, fi, _p(clip), _p(w16), _p(self.ema), ema_decay, st), "cc_adamw_step_ema")
        elif clip is not None:
            check(l.cc_adamw_step_clip(self.op_dtype, _p(p), _p(g), _p(m), _p(v), n, lr, betas[0], betas[1], eps, weight_decay, step, grad_scale,
                                       ls, fi, _p(clip), _p(w16), st), "cc_adamw_step_clip")
        elif w16 is None:
            check(l.cc_adamw_step(_p(p), _p(g), _p(m), _p(v), n, lr, betas[0], betas[1], eps, weight_decay, step, grad_scale, ls, fi, st),
                  "cc_adamw_step")
        else:
            check(l.cc_adamw_step_cast(self.op_dtype, _p(p), _p(g), _p(m), _p(v), n, lr, betas[0], betas[1], eps, weight_decay, step, grad_scale,
                                       ls, fi, _p(w16), st), "cc_adamw_step_cast")

    def grad_range(self, partitioned: bool) -> Tuple[int, int]:
        """[lo, hi) of the gradient arena whose reduced sum this rank holds: everything, or with partitioned gradients (ZeRO stage 2) the
        slice whose moments it owns."""
        if partitioned and self.zero is not None:
            return self.zero[1][self.zero[0]]
        return 0, self.n

    def adamw_step(self, lr: float, step: int, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, grad_scale: float = 1.0,
                   scaler: Optional["LossScaler"] = None, clip: Optional[torch.Tensor] = None, ema_decay: Optional[float] = None):
        """torch.optim.AdamW math (reference model.py:73-77) over the whole arena, refreshing the 16-bit operand copy.
        ``scaler`` (fp16 operands): the gradients carry its loss scale, and a step whose backward overflowed is skipped on the device.
        ``clip``: device float[1], the global-norm clip coefficient the gradients are also multiplied by (GradClipper.coef).
        ``ema_decay``: d in [0, 1) — the same launch also updates the weight average, ema = d * ema + (1 - d) * p over the parameters
        it just wrote (cc_adamw_step_ema; enabled at the current master on first use); a step skipped on the device skips the average,
        a sharded step averages the own slice.  None: exactly the launches of a step without the option."""
        ema_decay = check_ema_decay(ema_decay)
        if ema_decay is not None:
            self.enable_ema()
        kw = (lr, step, betas, eps, weight_decay, grad_scale, scaler, clip, ema_decay)
        if self.zero is not None:                       # sharded optimizer state: own slice, then the owners' slices travel
            rank, ranges, gather = self.zero
            lo, hi = ranges[rank]
            if self.m is None:
                self.m = torch.zeros(hi - lo, dtype=torch.float32, device=self.device)
                self.v = torch.zeros(hi - lo, dtype=torch.float32, device=self.device)
            assert self.m.numel() == hi - lo
            if hi > lo:
                self._adamw(self.w32[lo:hi], self.grads()[lo:hi], self.m, self.v, hi - lo, None, *kw)
            gather(self.w32, ranges)
            self.refresh_bf16()
            return
        if self.m is None:
            self.m = torch.zeros_like(self.w32)
            self.v = torch.zeros_like(self.w32)
        # The step also stores the 16-bit cast of every updated parameter (cc_adamw_step_cast), so the operand arena only needs its
        # transposed half rebuilt.  One corner keeps the full refresh: a step that may be SKIPPED on the device (fp16 overflow) leaves
        # the cast untouched, which is only right if the cast was current before the step.
        if os.environ.get("CC_ADAMW_TWO_PASS") or self.op_dtype == OP_X3:   # A/B switch: the separate-cast form; bf16x3: operand images are per matrix
            self._adamw(self.w32, self.grads(), self.m, self.v, self.n, None, *kw)
            self.refresh_bf16()
            return
        current = self._stamp() == self._w16_version
        self._adamw(self.w32, self.grads(), self.m, self.v, self.n, self.w16, *kw)
        if scaler is None or current:
            check(self.sync_fn(None, _p(self.w16), _stream(self.device)), "cc_*_transpose_weights")
            self._w16_version = self._stamp()
        else:
            self.refresh_bf16()


class LossScaler:
    """Dynamic loss scale for fp16-operand training, torch.cuda.amp.GradScaler semantics (init 2^16, x2 every 2000 good steps, x0.5
    on overflow) — what Lightning wraps around the reference's model for ``--fp-precision 16`` — kept entirely on the device:
    ``state`` = [scale, good-step counter, applied-step counter], ``found_inf`` is raised by cc_grad_nonfinite and read by cc_adamw_step (which then skips
    the step) and by cc_loss_scale_update.  No host synchronisation anywhere."""

    def __init__(self, device, init_scale: float = 65536.0, growth: float = 2.0, backoff: float = 0.5, interval: int = 2000):
        self.device = torch.device(device)
        # [scale, good steps since the last change, optimizer steps actually APPLIED (skipped ones do not count: Adam's bias correction
        # follows this counter, as torch.cuda.amp.GradScaler + torch.optim.AdamW do)]
        self.state = torch.tensor([init_scale, 0.0, 0.0], dtype=torch.float32, device=self.device)
        self.found_inf = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.growth, self.backoff, self.interval = growth, backoff, interval

    @property
    def scale(self) -> torch.Tensor:
        return self.state[0:1]

    def check(self, arena: "_Arena") -> None:
        """Raise found_inf if the arena's (scaled) gradients hold an inf / nan.  Multi-GPU: call after the all-reduce."""
        check(_lib.lib().cc_grad_nonfinite(_p(arena.grads()), arena.n, _p(self.found_inf), _stream(self.device)), "cc_grad_nonfinite")

    def update(self) -> None:
        """After the optimizer steps of this iteration: adjust the scale and clear found_inf."""
        check(_lib.lib().cc_loss_scale_update(_p(self.state), _p(self.found_inf), self.growth, self.backoff, self.interval,
                                              _stream(self.device)), "cc_loss_scale_update")


class GradClipper:
    """Global gradient-norm clipping, torch.nn.utils.clip_grad_norm_ semantics (what Lightning's ``gradient_clip_val`` gives the
    reference's trainer), kept entirely on the device: ``sumsq`` collects the squared norm of the trained arenas (cc_grad_sqnorm),
    ``clip`` = [coefficient min(1, max_norm / (norm + 1e-6)), norm] (cc_grad_clip_coef); cc_adamw_step_clip reads the coefficient.
    ``max_norm`` = inf reports the norm and clips nothing.  No host synchronisation anywhere."""

    def __init__(self, device, max_norm: float):
        self.device = torch.device(device)
        self.max_norm = float(max_norm)
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.clip = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.scratch = torch.empty(_lib.lib().cc_grad_norm_scratch_floats(), dtype=torch.float32, device=self.device)

    @property
    def coef(self) -> torch.Tensor:
        return self.clip[0:1]

    @property
    def norm(self) -> torch.Tensor:
        return self.clip[1:2]

    def begin(self) -> None:
        self.sumsq.zero_()

    def add(self, arena: "_Arena", lo: int = 0, hi: Optional[int] = None) -> None:
        """sumsq += the squared norm of elements [lo, hi) of the arena's (still loss-scaled) gradients."""
        hi = arena.n if hi is None else hi
        if hi > lo:
            check(_lib.lib().cc_grad_sqnorm(_p(arena.grads()[lo:hi]), hi - lo, _p(self.scratch), _p(self.sumsq), _stream(self.device)),
                  "cc_grad_sqnorm")

    def finish(self, grad_scale: float = 1.0, scaler: Optional[LossScaler] = None) -> None:
        check(_lib.lib().cc_grad_clip_coef(_p(self.sumsq), self.max_norm, grad_scale, _p(scaler.scale) if scaler is not None else None,
                                           _p(self.clip), _stream(self.device)), "cc_grad_clip_coef")


class MapperEngine:
    """TransformerMapper / TransformerMapperWindowed (reference clipcap/model/mapper.py:113-160) on the HIP library."""

    def __init__(self, E: int, D: int, prefix_length: int, projection_length: int, num_heads: int, num_layers: int, window: int = 1,
                 use_pos: bool = False, device="cpu", precision=None):
        self.dims = dict(E=E, D=D, P=projection_length, L=prefix_length, H=num_heads, N=num_layers, Hm=int(D * 2.0), W=window,
                         use_pos=int(bool(use_pos) and window > 1))
        self.op_dtype = op_dtype_of(precision)
        self.cfg = MapperCfg(op_dtype=self.op_dtype, **self.dims)
        l = _lib.lib()
        n = l.cc_mapper_param_count(C.byref(self.cfg))
        if n < 0:
            raise _lib.CCError(f"unsupported mapper configuration {self.dims}: dims must be multiples of 8 (head dim too)")
        self.arena = _Arena(n, device, self._sync, self.op_dtype)
        offs = (C.c_int64 * (4 + 12 * num_layers))()
        check(l.cc_mapper_param_offsets(C.byref(self.cfg), offs))
        self.offsets = list(offs)
        self._ws: Dict[Tuple[int, int], torch.Tensor] = {}

    def _sync(self, w32, w16, st):
        if w32 is None:          # the cast half is current (written by the optimizer step): transposed copies only
            return _lib.lib().cc_mapper_transpose_weights(C.byref(self.cfg), w16, st)
        return _lib.lib().cc_mapper_sync_weights(C.byref(self.cfg), w32, w16, st)

    # ---- named views (reference state-dict names / layouts) ----
    def shapes(self) -> List[Tuple[str, int, Tuple[int, ...]]]:
        d = self.dims
        E, D, P, L, N, Hm, W = d["E"], d["D"], d["P"], d["L"], d["N"], d["Hm"], d["W"]
        out = [("linear.weight", self.offsets[0], (P * D, E)), ("linear.bias", self.offsets[1], (P * D,)),
               ("prefix_const", self.offsets[2], (L, D))]
        if self.offsets[3] >= 0:
            out.append(("pos_embeddings", self.offsets[3], (W * P, D)))
        shp = [(D,), (D,), (D, D), (2 * D, D), (D, D), (D,), (D,), (D,), (Hm, D), (Hm,), (D, Hm), (D,)]
        for i in range(N):
            for j, nm in enumerate(MAPPER_LAYER_NAMES):
                out.append((f"transformer.layers.{i}.{nm}", self.offsets[4 + 12 * i + j], shp[j]))
        return out

    def views(self, arena: torch.Tensor) -> Dict[str, torch.Tensor]:
        res = {}
        for name, off, shape in self.shapes():
            n = 1
            for s in shape:
                n *= s
            res[name] = arena[off:off + n].view(shape)
        return res

    def to(self, device):
        device = torch.device(device)
        if device == self.arena.device:
            return self
        self.arena = self.arena.moved_to(device, self._sync)
        self._ws.clear()
        return self

    def set_precision(self, precision) -> None:
        """16 -> fp16 operands (the reference's --fp-precision 16), 32 / 64 -> split-bf16 operands (the reference's default precision),
        'bf16' -> bf16 operands (_lib.op_dtype_of).  fp32 master unchanged."""
        self.op_dtype = op_dtype_of(precision)
        self.cfg.op_dtype = self.op_dtype
        self.arena.set_op_dtype(self.op_dtype)
        self._ws.clear()

    def _workspace(self, B: int, save: int) -> torch.Tensor:
        key = (B, save)
        ws = self._ws.get(key)
        if ws is None:
            nbytes = _lib.lib().cc_mapper_ws_bytes(C.byref(self.cfg), B, save)
            check(nbytes, "cc_mapper_ws_bytes")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.arena.device)
            self._ws[key] = ws
        return ws

    def forward(self, emb: torch.Tensor, save: bool = False) -> torch.Tensor:
        """emb fp32 (B,E) or (B,W,E) -> prefix fp32 (B,L,D)."""
        _require_cuda(self.arena.w32, "MapperEngine.forward")
        d = self.dims
        emb = emb.to(device=self.arena.device, dtype=torch.float32).contiguous()
        B = emb.shape[0]
        if emb.numel() != B * d["W"] * d["E"]:
            raise ValueError(f"expected embeddings of shape ({B},{d['W']},{d['E']}), got {tuple(emb.shape)}")
        self.arena.sync_bf16()
        out = torch.empty(B, d["L"], d["D"], dtype=torch.float32, device=self.arena.device)
        ws = self._workspace(B, int(save))
        check(_lib.lib().cc_mapper_fwd(C.byref(self.cfg), B, _p(self.arena.w32), _p(self.arena.w16), _p(emb), _p(ws), _p(out), int(save),
                                      _stream(self.arena.device)), "cc_mapper_fwd")
        self._last = (B, emb)  # keep the input alive until backward has consumed the workspace
        if save:
            self._saved_batch = B
            self._fwd_serial = getattr(self, "_fwd_serial", 0) + 1
        return out

    def attention_probs(self, B: int) -> List[torch.Tensor]:
        """Per layer, the attention probabilities (B, S, S, H) of the last forward(save=True) with batch B — the second return value
        of the reference's MultiHeadAttention.forward (attention.py:32-42)."""
        ws = self._ws.get((B, 1))
        if ws is None or getattr(self, "_saved_batch", None) != B:
            raise RuntimeError("MapperEngine.attention_probs needs a preceding forward(save=True) with the same batch")
        d = self.dims
        S = d["W"] * d["P"] + d["L"]
        outs = []
        for l in range(d["N"]):
            out = torch.empty(B, S, S, d["H"], dtype=torch.float32, device=self.arena.device)
            check(_lib.lib().cc_mapper_attention_probs(C.byref(self.cfg), B, _p(ws), l, _p(out), _stream(self.arena.device)),
                  "cc_mapper_attention_probs")
            outs.append(out)
        return outs

    def layer_span(self, l: int) -> Tuple[int, int]:
        """[lo, hi) element range of layer l's parameters in the arenas (layers are contiguous, head tensors come first)."""
        lo = self.offsets[4 + 12 * l]
        hi = self.offsets[4 + 12 * (l + 1)] if l + 1 < self.dims["N"] else self.arena.n
        return lo, hi

    def backward(self, dout: torch.Tensor, on_layers_done=None, group: int = 2):
        """Accumulates d loss / d params into the gradient arena; needs a preceding forward(save=True).
        on_layers_done(lo, hi): called right after the kernels of a slice of layers are enqueued, with the arena element range
        whose gradients are then final — the hook the DDP reducer uses to overlap its all-reduce with the rest of backward."""
        B = dout.shape[0]
        dout = dout.to(dtype=torch.float32).contiguous()
        ws = self._ws.get((B, 1))
        if ws is None:
            raise RuntimeError("MapperEngine.backward without forward(save=True)")
        l = _lib.lib()
        a = self.arena
        N = self.dims["N"]
        if on_layers_done is None:
            check(l.cc_mapper_bwd(C.byref(self.cfg), B, _p(a.w32), _p(a.w16), _p(ws), _p(dout), _p(a.grads()), _stream(a.device)), "cc_mapper_bwd")
            return
        hi = N
        while hi > 0:
            lo = max(0, hi - group)
            check(l.cc_mapper_bwd_range(C.byref(self.cfg), B, _p(a.w32), _p(a.w16), _p(ws), _p(dout), _p(a.grads()), hi, lo, _stream(a.device)),
                  "cc_mapper_bwd_range")
            if lo > 0:
                on_layers_done(self.layer_span(lo)[0], self.layer_span(hi - 1)[1])
            else:   # the l_lo == 0 call also produced the head tensors' gradients
                on_layers_done(0, self.layer_span(hi - 1)[1])
            hi = lo
        if N == 0:
            check(l.cc_mapper_bwd_range(C.byref(self.cfg), B, _p(a.w32), _p(a.w16), _p(ws), _p(dout), _p(a.grads()), 0, 0, _stream(a.device)),
                  "cc_mapper_bwd_range")
            on_layers_done(0, a.n)


class MlpMapperEngine:
    """The MLP mapping network of the ClipCap paper — Linear(E -> L*D/2), Tanh, Linear(L*D/2 -> L*D), reshaped to (B, L, D) — on the
    HIP library (cc_mlp_*).  Same engine interface as MapperEngine where its callers use it (ClipCapEngine, GradReducer, the
    checkpoint callback, EMA, the decoders); state-dict names are the original's nn.Sequential indices."""

    NAMES = ("model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias")

    def __init__(self, E: int, D: int, prefix_length: int, device="cpu", precision=None):
        L = prefix_length
        if (L * D) % 2:
            raise _lib.CCError(f"unsupported MLP mapper configuration E={E} D={D} L={L}: L*D must be even (hidden width L*D/2)")
        self.dims = dict(E=E, D=D, L=L, Hd=(L * D) // 2, W=1)
        self.op_dtype = op_dtype_of(precision)
        self.cfg = _lib.MlpCfg(E=E, D=D, L=L, Hd=self.dims["Hd"], op_dtype=self.op_dtype)
        l = _lib.lib()
        n = l.cc_mlp_param_count(C.byref(self.cfg))
        if n < 0:
            raise _lib.CCError(f"unsupported MLP mapper configuration {self.dims}: E, D and L*D/2 must be multiples of 8")
        self.arena = _Arena(n, device, self._sync, self.op_dtype)
        offs = (C.c_int64 * 4)()
        check(l.cc_mlp_param_offsets(C.byref(self.cfg), offs))
        self.offsets = list(offs)
        self._ws: Dict[Tuple[int, int], torch.Tensor] = {}

    def _sync(self, w32, w16, st):
        if w32 is None:          # the cast half is current (written by the optimizer step): transposed copy only
            return _lib.lib().cc_mlp_transpose_weights(C.byref(self.cfg), w16, st)
        return _lib.lib().cc_mlp_sync_weights(C.byref(self.cfg), w32, w16, st)

    def shapes(self) -> List[Tuple[str, int, Tuple[int, ...]]]:
        d = self.dims
        E, LD, Hd = d["E"], d["L"] * d["D"], d["Hd"]
        shp = [(Hd, E), (Hd,), (LD, Hd), (LD,)]
        return [(nm, self.offsets[i], shp[i]) for i, nm in enumerate(self.NAMES)]

    views = MapperEngine.views
    to = MapperEngine.to
    set_precision = MapperEngine.set_precision

    def _workspace(self, B: int, save: int) -> torch.Tensor:
        key = (B, save)
        ws = self._ws.get(key)
        if ws is None:
            nbytes = _lib.lib().cc_mlp_ws_bytes(C.byref(self.cfg), B, save)
            check(nbytes, "cc_mlp_ws_bytes")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.arena.device)
            self._ws[key] = ws
        return ws

    def forward(self, emb: torch.Tensor, save: bool = False) -> torch.Tensor:
        """emb fp32 (B, E) -> prefix fp32 (B, L, D)."""
        d = self.dims
        if emb.dim() != 2 or emb.shape[1] != d["E"]:
            raise ValueError(f"expected embeddings of shape (B,{d['E']}), got {tuple(emb.shape)} (the MLP mapper takes no windowed embeddings)")
        _require_cuda(self.arena.w32, "MlpMapperEngine.forward")
        emb = emb.to(device=self.arena.device, dtype=torch.float32).contiguous()
        B = emb.shape[0]
        self.arena.sync_bf16()
        out = torch.empty(B, d["L"], d["D"], dtype=torch.float32, device=self.arena.device)
        ws = self._workspace(B, int(save))
        check(_lib.lib().cc_mlp_fwd(C.byref(self.cfg), B, _p(self.arena.w32), _p(self.arena.w16), _p(emb), _p(ws), _p(out), int(save),
                                   _stream(self.arena.device)), "cc_mlp_fwd")
        self._last = (B, emb)  # keep the input alive until backward has consumed the workspace
        if save:
            self._saved_batch = B
            self._fwd_serial = getattr(self, "_fwd_serial", 0) + 1
        return out

    def get(self, B: int, field: int) -> torch.Tensor:
        """Test hook (cc_mlp_get): one saved field of the last forward(save=True) / backward with batch B, in its stored type:
        0 x16 (B, E), 1 h (B, Hd), 2 t (B, Hd), 3 g16 (B, L*D), 4 dU (B, Hd)."""
        ws = self._ws.get((B, 1))
        if ws is None:
            raise RuntimeError("MlpMapperEngine.get needs a preceding forward(save=True) with the same batch")
        d = self.dims
        width = (d["E"], d["Hd"], d["Hd"], d["L"] * d["D"], d["Hd"])[field]
        dt = {OP_BF16: torch.bfloat16, OP_FP16: torch.float16, OP_X3: torch.float32}[self.op_dtype]
        out = torch.empty(B, width, dtype=dt, device=self.arena.device)
        check(_lib.lib().cc_mlp_get(C.byref(self.cfg), B, _p(ws), field, _p(out), out.numel() * out.element_size(), _stream(self.arena.device)),
              "cc_mlp_get")
        return out

    def backward(self, dout: torch.Tensor, on_layers_done=None, group: int = 2):
        """Accumulates d loss / d params into the gradient arena; needs a preceding forward(save=True).  No gradient for the input.
        on_layers_done(lo, hi): with it the pass runs in two halves — model.2.* first (94 % of the gradient bytes at the real shape),
        reported as [off(model.2.weight), n), then model.0.*, reported as [0, off(model.2.weight)) — so the DDP reducer has most of
        the arena on the wire before the second half is enqueued.  `group` is accepted for MapperEngine's signature and unused."""
        B = dout.shape[0]
        dout = dout.to(dtype=torch.float32).contiguous()
        ws = self._ws.get((B, 1))
        if ws is None:
            raise RuntimeError("MlpMapperEngine.backward without forward(save=True)")
        l = _lib.lib()
        a = self.arena
        args = (C.byref(self.cfg), B, _p(a.w32), _p(a.w16), _p(ws), _p(dout), _p(a.grads()))
        if on_layers_done is None:
            check(l.cc_mlp_bwd(*args, _stream(a.device)), "cc_mlp_bwd")
            return
        cut = self.offsets[2]
        check(l.cc_mlp_bwd_part(*args, 1, _stream(a.device)), "cc_mlp_bwd_part")
        on_layers_done(cut, a.n)
        check(l.cc_mlp_bwd_part(*args, 0, _stream(a.device)), "cc_mlp_bwd_part")
        on_layers_done(0, cut)


class Gpt2Engine:
    """HF GPT2LMHeadModel arithmetic (transformers modeling_gpt2.py) on the HIP library; arena keeps HF layouts."""

    def __init__(self, n_embd: int, n_head: int, n_layer: int, vocab_size: int, n_positions: int, device="cpu", precision=None):
        self.dims = dict(D=n_embd, H=n_head, NL=n_layer, V=vocab_size, Vp=(vocab_size + 127) // 128 * 128, NPOS=n_positions)
        self.op_dtype = op_dtype_of(precision)
        self.cfg = Gpt2Cfg(op_dtype=self.op_dtype, **self.dims)
        l = _lib.lib()
        n = l.cc_gpt2_param_count(C.byref(self.cfg))
        if n < 0:
            raise _lib.CCError(f"unsupported GPT-2 configuration {self.dims}")
        self.arena = _Arena(n, device, self._sync, self.op_dtype)
        offs = (C.c_int64 * (2 + 12 * n_layer + 2))()
        check(l.cc_gpt2_param_offsets(C.byref(self.cfg), offs))
        self.offsets = list(offs)
        self._ws: Dict[int, torch.Tensor] = {}

    def _sync(self, w32, w16, st):
        if w32 is None:
            return _lib.lib().cc_gpt2_transpose_weights(C.byref(self.cfg), w16, st)
        return _lib.lib().cc_gpt2_sync_weights(C.byref(self.cfg), w32, w16, st)

    def decode_images(self) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """LAB LIBRARY ONLY (CLIPCAP_HIP_LIB=lab; (None, None) with the product library).  (wimg, wteam) for cc_decode_fwd_x
        (include/clipcap_hip_lab.h), rebuilt whenever the operand copy changes:
        wimg  — the block GEMM weights in MFMA fragment order (cc_decode_image; cc_decode_mode bit 3): the decode GEMMs whose K is split over
                the waves load the weight operand global -> VGPR from it;
        wteam — the XCD-team engine's image (cc_decode_xt_image; lab build, cc_decode_mode bit 2).
        None where the library does not cover this model (width, operand type), the switch is off, or the build lacks the engine."""
        a = self.arena
        if not _lib.IS_LAB:
            return None, None
        l = _lib.lib()
        mode = l.cc_decode_mode(-1)
        if a.device.type != "cuda" or not (mode & 12):
            return None, None
        a.sync_bf16()
        key = (a._w16_version, a.op_dtype, a.w16.data_ptr(), mode & 12)
        if getattr(self, "_img_key", None) != key:
            out = []
            for bit, nbytes_fn, build_fn, name in ((8, l.cc_decode_image_bytes, l.cc_decode_image, "cc_decode_image"),
                                                  (4, l.cc_decode_xt_image_bytes, l.cc_decode_xt_image, "cc_decode_xt_image")):
                nbytes = nbytes_fn(C.byref(self.cfg)) if mode & bit else 0
                if nbytes <= 0:
                    out.append(None)
                    continue
                img = torch.empty(nbytes // 2, dtype=a.w16.dtype, device=a.device)
                check(build_fn(C.byref(self.cfg), _p(a.w16), _p(img), _stream(a.device)), name)
                out.append(img)
            self._imgs = tuple(out)
            self._img_key = key
        return self._imgs

    def shapes(self) -> List[Tuple[str, int, Tuple[int, ...]]]:
        d = self.dims
        D, NL, V, NPOS = d["D"], d["NL"], d["V"], d["NPOS"]
        out = [("transformer.wte.weight", self.offsets[0], (V, D)), ("transformer.wpe.weight", self.offsets[1], (NPOS, D))]
        shp = [(D,), (D,), (D, 3 * D), (3 * D,), (D, D), (D,), (D,), (D,), (D, 4 * D), (4 * D,), (4 * D, D), (D,)]
        for i in range(NL):
            for j, nm in enumerate(GPT2_LAYER_NAMES):
                out.append((f"transformer.h.{i}.{nm}", self.offsets[2 + 12 * i + j], shp[j]))
        out.append(("transformer.ln_f.weight", self.offsets[2 + 12 * NL], (D,)))
        out.append(("transformer.ln_f.bias", self.offsets[3 + 12 * NL], (D,)))
        return out

    views = MapperEngine.views
    to = MapperEngine.to
    set_precision = MapperEngine.set_precision

    def layer_span(self, l: int) -> Tuple[int, int]:
        lo = self.offsets[2 + 12 * l]
        hi = self.offsets[2 + 12 * (l + 1)]      # the entry after the last layer is ln_f.weight
        return lo, hi

    def shape(self, B: int, L: int, T: int, cap: int, mode: int, dropout=None) -> Gpt2Shape:
        """dropout: optional (p_embd, p_attn, p_resid, seed) of this pass (full finetune in train mode); None = eval behaviour."""
        if dropout is None:
            return Gpt2Shape(B, L, T, cap, mode, 0.0, 0.0, 0.0, 0)
        return Gpt2Shape(B, L, T, cap, mode, float(dropout[0]), float(dropout[1]), float(dropout[2]), int(dropout[3]) & 0xFFFFFFFFFFFFFFFF)

    def workspace(self, shp: Gpt2Shape) -> torch.Tensor:
        """One buffer per mode, grown on demand: the library carves its layout from the base pointer on every call, so a buffer
        sized for the largest shape seen serves all smaller ones (caption length varies from batch to batch in real training)."""
        nbytes = _lib.lib().cc_gpt2_ws_bytes(C.byref(self.cfg), C.byref(shp))
        check(nbytes, "cc_gpt2_ws_bytes")
        ws = self._ws.get(shp.mode)
        if ws is None or ws.numel() < nbytes or ws.device != self.arena.device:
            self._ws.pop(shp.mode, None)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.arena.device)
            self._ws[shp.mode] = ws
        # every hand-out of a mode's buffer may overwrite the activations a differentiable .logits pass left in it: the autograd
        # bridge compares this counter (logits(save_mode) / logits_backward)
        self._ws_uses = getattr(self, "_ws_uses", 0) + 1
        return ws

    # -- inference-style forward: logits for all rows (ClipCapModel.forward / language_model(inputs_embeds=...)) --
    def logits(self, inputs_embeds: torch.Tensor, save_mode: int = 0) -> torch.Tensor:
        """inputs_embeds fp32 (B,T,D) (no positional embedding) -> fp32 logits (B,T,V).  save_mode 1 / 2 keeps the activations for
        logits_backward (1: gradient wrt inputs_embeds only, 2: + every GPT-2 weight gradient)."""
        _require_cuda(self.arena.w32, "Gpt2Engine.logits")
        l = _lib.lib()
        x = inputs_embeds.to(device=self.arena.device, dtype=torch.float32).contiguous()
        B, T, D = x.shape
        shp = self.shape(B, T, T, 0, 0) if not save_mode else self.shape(B, 0, T, T, save_mode)
        if save_mode:
            self._logits_pass = (shp, getattr(self, "_logits_pass", (None, 0, 0))[1] + 1, 0)
        ws = self.workspace(shp)
        self.arena.sync_bf16()
        st = _stream(self.arena.device)
        a = self.arena
        check(l.cc_gpt2_embed_from(C.byref(self.cfg), C.byref(shp), _p(a.w32), _p(x), _p(ws), st), "cc_gpt2_embed_from")
        check(l.cc_gpt2_fwd(C.byref(self.cfg), C.byref(shp), _p(a.w32), _p(a.w16), _p(ws), st), "cc_gpt2_fwd")
        Vp = self.dims["Vp"]
        out = torch.empty(B * T, Vp, dtype=torch.float32, device=a.device)
        check(l.cc_gpt2_logits(C.byref(self.cfg), C.byref(shp), _p(a.w32), _p(a.w16), _p(ws), _p(out), Vp, st), "cc_gpt2_logits")
        if save_mode:
            self._logits_pass = (shp, self._logits_pass[1], self._ws_uses)
        return out.view(B, T, Vp)[:, :, : self.dims["V"]]

    def logits_backward(self, dlogits: torch.Tensor) -> torch.Tensor:
        """d loss / d inputs_embeds (B,T,D) for the last logits(..., save_mode >= 1) pass; save_mode 2 also ACCUMULATES the GPT-2 weight
        gradients into the arena's g32 (cc_gpt2_logits_bwd)."""
        shp, _, uses = self._logits_pass
        if uses != self._ws_uses:
            raise RuntimeError("Gpt2Engine.logits_backward: another pass has used the activation workspace since the forward; "
                               "call backward() before running the language model again")
        a = self.arena
        dl = dlogits.to(device=a.device, dtype=torch.float32).contiguous()
        B, T, V = dl.shape
        assert (B, T) == (shp.B, shp.T) and V == self.dims["V"]
        dx0 = torch.empty(B, T, self.dims["D"], dtype=torch.float32, device=a.device)
        ws = self.workspace(shp)
        scale = keep = None
        if self.op_dtype == OP_FP16:
            # fp16 operands: d logits of a mean cross-entropy are p / N ~ 1e-9 .. 1e-5, below fp16's normal range (6e-5) — the whole
            # backward runs under a power-of-two scale chosen on the device from max |d logits| (no host sync) and divided out of dx0
            # and of the weight gradients afterwards, as the fused trainer does with its LossScaler
            amax = dl.abs().amax().clamp_min(1e-30)
            scale = torch.exp2(torch.floor(torch.log2(256.0 / amax)))
            dl = dl * scale
            if shp.mode == 2:
                keep = a.grads().clone()
                a.grads().zero_()
        check(_lib.lib().cc_gpt2_logits_bwd(C.byref(self.cfg), C.byref(shp), _p(a.w32), _p(a.w16), _p(ws), _p(dl), V, _p(dx0),
                                            _p(a.grads()) if shp.mode == 2 else None, _stream(a.device)), "cc_gpt2_logits_bwd")
        if scale is not None:
            dx0 = dx0 / scale
            if keep is not None:
                a.grads().div_(scale).add_(keep)
        return dx0


def check_label_smoothing(eps) -> float:
    """eps of a label-smoothed loss as a float in [0, 1); ValueError otherwise (NaN included), before anything is launched"""
    e = float(eps)
    if not 0.0 <= e < 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1), got {eps!r}")
    return e


def check_ema_decay(value) -> Optional[float]:
    """decay of the weight average: None (no average) or a float in [0, 1); ValueError otherwise (NaN included), before an engine, the
    library or a device is touched"""
    if value is None:
        return None
    d = float(value)
    if not 0.0 <= d < 1.0:
        raise ValueError(f"ema_decay must be None or lie in [0, 1), got {value!r}")
    return d


def ema_decay_at(decay: float, t: int, warmup: bool) -> float:
    """d_t of optimizer step t (1-based, the host's count): ``decay``, or with warm-up min(decay, (1 + t) / (10 + t)) — the average
    forgets its starting point quickly while the weights still move fast"""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def check_token_weights(token_weights, shape, name: str = "token_weights") -> None:
    """A per-token loss weight tensor is fp32 of ``shape``; ValueError otherwise.  Looks at the type, dtype and shape only: the values
    stay on whatever device they are (no host sync), any finite value of either sign is allowed and the weight of an ignored position
    is never used."""
    if not isinstance(token_weights, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor, got {type(token_weights).__name__}")
    if token_weights.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {token_weights.dtype}")
    if tuple(token_weights.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(token_weights.shape)}")


class ClipCapEngine:
    """Training step of ClipCapModel (reference model.py:94-113) as straight-line forward + backward kernel chains."""

    def __init__(self, mapper: MapperEngine, gpt2: Gpt2Engine, train_lm: bool):
        self.mapper = mapper
        self.gpt2 = gpt2
        self.train_lm = train_lm
        self.stats: Optional[torch.Tensor] = None
        # fp16 operands: the backward pass runs under a dynamic loss scale (gradients in g32 are scale x the true ones until
        # optimizer_step divides it out); bf16 operands need none
        self.scaler: Optional[LossScaler] = None
        # global-norm clipping (optimizer_step(max_grad_norm=...)): built on first use; last_grad_norm views its device-side norm
        self.clipper: Optional[GradClipper] = None
        self.last_grad_norm: Optional[torch.Tensor] = None
        # label smoothing (forward_backward(label_smoothing=...)): the 3-float stats and the scratch of cc_lmhead_ce_*_smooth, built on
        # first use; last_nll = the mean plain NLL of the last step (a device scalar; equal to the returned loss without smoothing)
        self.stats3: Optional[torch.Tensor] = None
        self.smooth_scratch: Optional[torch.Tensor] = None
        self.last_nll: Optional[torch.Tensor] = None

    def _clipper(self, dev, max_norm: float) -> GradClipper:
        if self.clipper is None or self.clipper.device != dev:
            self.clipper = GradClipper(dev, max_norm)
            self.last_grad_norm = self.clipper.norm
        self.clipper.max_norm = float(max_norm)
        return self.clipper

    def _scaler(self, dev) -> Optional[LossScaler]:
        if OP_FP16 not in (self.gpt2.op_dtype, self.mapper.op_dtype):
            return None
        if self.scaler is None or self.scaler.device != dev:
            self.scaler = LossScaler(dev)
        return self.scaler

    def arenas(self) -> List[_Arena]:
        return [self.mapper.arena] + ([self.gpt2.arena] if self.train_lm else [])

    def optimizer_step(self, lr: float, step: int, sync_flag=None, max_grad_norm: Optional[float] = None, sync_norm=None, **adamw_kw) -> None:
        """AdamW over every trained arena (reference model.py:67-91).  With fp16 operands: overflow check of the scaled gradients
        (after any all-reduce), the step is skipped on the device if they overflowed, then the loss scale is adjusted.
        ``sync_flag(found_inf)``: optional in-place SUM over the ranks (ddp.GradReducer.reduce_flag) — with partitioned gradients
        (ZeRO stage 2) a rank only sees its own slice summed, so the ranks agree on the overflow flag before anyone steps.
        ``max_grad_norm``: clip the gradients of all trained arenas together to this global 2-norm (clip_grad_norm_'s rule; inf: only
        measure it) and leave the norm on the device in ``last_grad_norm``; None: the step launches exactly what it launched without
        this option.  ``sync_norm(sumsq)``: the same in-place 1-float SUM over the ranks, given exactly when the gradients are
        partitioned — each rank then squares only the slice it owns; with whole reduced arenas every rank computes the same bits alone.
        ``ema_decay`` (forwarded to every trained arena's adamw_step with the other ``adamw_kw``): d in [0, 1) — each arena's weight
        average is updated inside its AdamW launch, ema = d * ema + (1 - d) * p; a step the loss scaler skips leaves it untouched."""
        sc = self.scaler
        if sc is not None:
            for a in self.arenas():
                sc.check(a)
            if sync_flag is not None:
                sync_flag(sc.found_inf)
        if max_grad_norm is not None:
            cl = self._clipper(self.arenas()[0].device, max_grad_norm)
            cl.begin()
            for a in self.arenas():
                cl.add(a, *a.grad_range(sync_norm is not None))
            if sync_norm is not None:
                sync_norm(cl.sumsq)
            cl.finish(adamw_kw.get("grad_scale", 1.0), sc)
            adamw_kw = dict(adamw_kw, clip=cl.coef)
        for a in self.arenas():
            a.adamw_step(lr, step, scaler=sc, **adamw_kw)
        if sc is not None:
            sc.update()

    def forward_backward(self, tokens: torch.Tensor, embeds: torch.Tensor, reduce_stats=None, backward: bool = True,
                         on_grads_ready=None, dropout=None, label_smoothing: float = 0.0,
                         token_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tokens int64 (B,cap) padded with -1; embeds fp32 (B,E)/(B,W,E).

        Returns the mean loss over kept targets (device scalar).  Gradients are ACCUMULATED into the arenas' g32.
        ``reduce_stats(stats)``: optional in-place all-reduce of the 2-float [loss_sum, kept_count] tensor, so the divisor is the
        global kept-token count (N-rank == 1-rank gradients).
        ``on_grads_ready(arena_index, lo, hi)``: optional; called as soon as the kernels producing gradient elements [lo, hi) of
        arena 0 (mapper) / 1 (GPT-2) are enqueued, in the order backward finishes them (GPT-2 top layers first, mapper last), so
        the caller can launch the all-reduce of that slice underneath the remaining backward kernels.
        ``dropout``: optional (p_embd, p_attn, p_resid, seed) — GPT-2 train-mode dropout for this step (full finetune; the masks
        are a hash of (seed, site, layer, element) regenerated by the backward kernels; the setting travels in this pass's
        cc_gpt2_shape, so concurrent engines on other streams are unaffected).
        With fp16 operands the gradients left in the arenas are multiplied by the current loss scale (self.scaler.scale);
        optimizer_step() divides it out.
        ``label_smoothing``: eps in [0, 1) of F.cross_entropy(..., ignore_index=0, label_smoothing=eps) over the real vocabulary.  0.0
        makes exactly the calls (and the 2-float stats) of a step without the option; a positive value goes through
        cc_lmhead_ce_fwd_smooth / cc_lmhead_ce_bwd_smooth with a 3-float stats [smoothed loss sum, kept count, plain NLL sum], returns
        the smoothed mean as torch does and leaves the mean plain NLL (what perplexity is made of) in ``last_nll``, a device scalar.
        ``token_weights``: fp32 (B, cap), a weight per target token: loss = sum over kept targets of weight * row loss / the kept COUNT
        (not the weight sum; under ``reduce_stats`` the global count).  Any finite value: negative (self-critical training), zero (the
        token still counts), large; the weight of an ignored target (token 0 or the -1 padding) is never used, whatever its bits.  None
        makes exactly the calls of a step without the option; a tensor goes through cc_lmhead_ce_fwd_w / cc_lmhead_ce_bwd_w (with
        ``label_smoothing`` as their eps) and the 3-float stats; the returned loss is the weighted mean, ``last_nll`` the plain one.
        """
        eps = check_label_smoothing(label_smoothing)
        if token_weights is not None:
            check_token_weights(token_weights, tokens.shape)
        l = _lib.lib()
        g, m = self.gpt2, self.mapper
        dev = g.arena.device
        _require_cuda(g.arena.w32, "ClipCapEngine.forward_backward")
        tokens = tokens.to(device=dev, dtype=torch.int64).contiguous()
        B, cap = tokens.shape
        L = m.dims["L"]
        T = L + cap
        mode = 2 if self.train_lm else 1
        shp = g.shape(B, L, T, cap, mode, dropout)
        ws = g.workspace(shp)
        g.arena.sync_bf16()
        st = _stream(dev)
        ga = g.arena
        prefix = m.forward(embeds, save=True)
        if token_weights is not None:
            token_weights = token_weights.to(device=dev).contiguous()
        return self._forward_backward(l, g, m, ga, shp, ws, st, prefix, tokens, reduce_stats, backward, on_grads_ready, dev, eps, token_weights)

    def _smooth_buffers(self, l, g, shp, dev) -> Tuple[torch.Tensor, torch.Tensor]:
        """(3-float stats, scratch) of the label-smoothed loss: the caller's buffers of cc_lmhead_ce_*_smooth, kept between steps"""
        n = check(l.cc_lmhead_smooth_scratch_floats(C.byref(g.cfg), C.byref(shp)), "cc_lmhead_smooth_scratch_floats")
        if self.stats3 is None or self.stats3.device != dev:
            self.stats3 = torch.zeros(3, dtype=torch.float32, device=dev)
        if self.smooth_scratch is None or self.smooth_scratch.device != dev or self.smooth_scratch.numel() < n:
            self.smooth_scratch = torch.empty(n, dtype=torch.float32, device=dev)
        return self.stats3, self.smooth_scratch

    def _forward_backward(self, l, g, m, ga, shp, ws, st, prefix, tokens, reduce_stats, backward, on_grads_ready, dev, eps=0.0, rw=None):
        check(l.cc_gpt2_embed(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(prefix), _p(tokens), _p(ws), st), "cc_gpt2_embed")
        check(l.cc_gpt2_fwd(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(ga.w16), _p(ws), st), "cc_gpt2_fwd")
        if rw is not None:
            stats, scratch = self._smooth_buffers(l, g, shp, dev)
            check(l.cc_lmhead_ce_fwd_w(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(ga.w16), _p(ws), _p(tokens), _p(rw), eps, _p(scratch),
                                       _p(stats), st), "cc_lmhead_ce_fwd_w")
        elif eps > 0.0:
            stats, scratch = self._smooth_buffers(l, g, shp, dev)
            check(l.cc_lmhead_ce_fwd_smooth(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(ga.w16), _p(ws), _p(tokens), eps, _p(scratch),
                                            _p(stats), st), "cc_lmhead_ce_fwd_smooth")
        else:
            if self.stats is None or self.stats.device != dev:
                self.stats = torch.zeros(2, dtype=torch.float32, device=dev)
            stats = self.stats
            check(l.cc_lmhead_ce_fwd(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(ga.w16), _p(ws), _p(tokens), _p(stats), st), "cc_lmhead_ce_fwd")
        if reduce_stats is not None:
            reduce_stats(stats)
        if backward:
            g32 = ga.grads() if self.train_lm else None
            denom = stats[1:2]
            sc = self._scaler(dev)
            if rw is not None:
                check(l.cc_lmhead_ce_bwd_w(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(ga.w16), _p(ws), _p(denom),
                                           _p(sc.scale) if sc is not None else None, _p(rw), eps, _p(scratch), _p(g32), st), "cc_lmhead_ce_bwd_w")
            elif eps > 0.0:
                check(l.cc_lmhead_ce_bwd_smooth(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(ga.w16), _p(ws), _p(denom),
                                                _p(sc.scale) if sc is not None else None, eps, _p(scratch), _p(g32), st), "cc_lmhead_ce_bwd_smooth")
            else:
                check(l.cc_lmhead_ce_bwd(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(ga.w16), _p(ws), _p(denom),
                                         _p(sc.scale) if sc is not None else None, _p(g32), st), "cc_lmhead_ce_bwd")
            dprefix = torch.empty_like(prefix)
            if on_grads_ready is None or not self.train_lm:
                check(l.cc_gpt2_bwd(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(ga.w16), _p(ws), _p(tokens), _p(dprefix), _p(g32), st), "cc_gpt2_bwd")
            else:
                NL, grp = g.dims["NL"], 2
                on_grads_ready(1, g.layer_span(NL - 1)[1], ga.n)                    # ln_f (from cc_lmhead_ce_bwd)
                hi = NL
                while hi > 0:
                    lo = max(0, hi - grp)
                    check(l.cc_gpt2_bwd_range(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(ga.w16), _p(ws), _p(tokens), _p(dprefix), _p(g32),
                                              hi, lo, st), "cc_gpt2_bwd_range")
                    on_grads_ready(1, g.layer_span(lo)[0] if lo > 0 else 0, g.layer_span(hi - 1)[1])   # lo == 0: + wte / wpe
                    hi = lo
            m.backward(dprefix, on_layers_done=(None if on_grads_ready is None else (lambda lo, hi: on_grads_ready(0, lo, hi))))
        loss = stats[0] / stats[1].clamp_min(1.0)
        self.last_nll = loss if (eps == 0.0 and rw is None) else stats[2] / stats[1].clamp_min(1.0)
        return loss

    @torch.no_grad()
    def score(self, tokens: torch.Tensor, embeds: Optional[torch.Tensor] = None, *, prefix: Optional[torch.Tensor] = None,
              ignore_zero: bool = False, chunk: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Teacher-forced log-likelihood of every caption under the model: a forward-only pass (mode 0: one layer's activations, eval
        behaviour, no dropout) whose lm_head stores no logits (cc_lmhead_score).

        tokens int64 (B, cap) padded with -1, as forward_backward takes them.  Exactly one of ``embeds`` (encoder embeddings (B, E) /
        (B, W, E): the mapper runs without saving) and ``prefix`` (fp32 (B, L, D), any L >= 1: an already mapped prefix, with a text
        prefix's embeddings appended if the caller wants one).
        Returns (token_logprob (B, cap): log p(tokens[b, c] | prefix, tokens[b, :c]) at kept positions and 0 elsewhere,
        sample_sum (B,), sample_count (B,)).  Kept: tokens >= 0; with ``ignore_zero`` also != 0 (the training loss's ignore_index).
        ``chunk``: samples per library call, bounding the workspace (default: the whole batch).
        Uses a workspace of its own and leaves ``stats``, the gradient arenas and the training workspaces alone, so it may run between
        forward_backward and optimizer_step.  With ``embeds`` the mapper's non-saving forward runs in the mapper's save = 0 workspace;
        the activations and the input a forward(save=True) keeps for MapperEngine.backward are left as they are."""
        if (embeds is None) == (prefix is None):
            raise ValueError("ClipCapEngine.score takes exactly one of embeds and prefix")
        l = _lib.lib()
        g, m = self.gpt2, self.mapper
        dev = g.arena.device
        _require_cuda(g.arena.w32, "ClipCapEngine.score")
        tokens = tokens.to(device=dev, dtype=torch.int64).contiguous()
        if tokens.dim() != 2 or tokens.shape[0] < 1 or tokens.shape[1] < 1:
            raise ValueError(f"tokens must be (B, cap) with B, cap >= 1, got {tuple(tokens.shape)}")
        B, cap = tokens.shape
        if prefix is not None:
            prefix = prefix.to(device=dev, dtype=torch.float32).contiguous()
            if prefix.dim() != 3 or prefix.shape[0] != B or prefix.shape[1] < 1 or prefix.shape[2] != g.dims["D"]:
                raise ValueError(f"prefix must be ({B}, L >= 1, {g.dims['D']}), got {tuple(prefix.shape)}")
            L = prefix.shape[1]
        else:
            embeds = embeds.to(device=dev, dtype=torch.float32)
            if embeds.shape[0] != B:
                raise ValueError(f"embeds has {embeds.shape[0]} rows for {B} token rows")
            L = m.dims["L"]
        T = L + cap
        if T > g.dims["NPOS"]:
            raise ValueError(f"prefix ({L}) + caption ({cap}) positions exceed n_positions = {g.dims['NPOS']}")
        out = torch.empty(B, cap, dtype=torch.float32, device=dev)
        stats = torch.empty(B, 2, dtype=torch.float32, device=dev)
        step = B if chunk is None else max(1, int(chunk))
        g.arena.sync_bf16()
        st = _stream(dev)
        ga = g.arena
        for lo in range(0, B, step):
            hi = min(B, lo + step)
            if prefix is not None:
                pre = prefix[lo:hi]
            else:
                kept_alive = getattr(m, "_last", None)      # the input a saved forward holds until its backward has run
                pre = m.forward(embeds[lo:hi], save=False)
                if kept_alive is not None:
                    m._last = kept_alive
            shp = g.shape(hi - lo, L, T, cap, 0)
            ws = self._score_workspace(shp)
            tk = tokens[lo:hi]
            check(l.cc_gpt2_embed(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(pre), _p(tk), _p(ws), st), "cc_gpt2_embed")
            check(l.cc_gpt2_fwd(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(ga.w16), _p(ws), st), "cc_gpt2_fwd")
            check(l.cc_lmhead_score(C.byref(g.cfg), C.byref(shp), _p(ga.w32), _p(ga.w16), _p(ws), _p(tk), int(bool(ignore_zero)), _p(out[lo:hi]),
                                    _p(stats[lo:hi]), st), "cc_lmhead_score")
        return out, stats[:, 0].contiguous(), stats[:, 1].contiguous()

    def _score_workspace(self, shp: Gpt2Shape) -> torch.Tensor:
        """The scoring pass's own buffer (grown on demand, like Gpt2Engine.workspace; never one of the engine's per-mode buffers)."""
        g = self.gpt2
        nbytes = _lib.lib().cc_gpt2_ws_bytes(C.byref(g.cfg), C.byref(shp))
        check(nbytes, "cc_gpt2_ws_bytes")
        ws = getattr(self, "_score_ws", None)
        if ws is None or ws.numel() < nbytes or ws.device != g.arena.device:
            self._score_ws = None
            ws = self._score_ws = torch.empty(nbytes, dtype=torch.uint8, device=g.arena.device)
        return ws

    def zero_grad(self):
        if self.mapper.arena.g32 is not None:
            self.mapper.arena.g32.zero_()
        if self.train_lm and self.gpt2.arena.g32 is not None:
            self.gpt2.arena.g32.zero_()


class DecodeSession:
    """KV-cached GPT-2 decode state for R rows (replaces the per-step full re-forward of the reference's inference/base.py:81).
    The cache is bf16 [n_layer][2][R][ctx_max][D], owned here.  A beam reorder (base.py:93,113) does not move cache data: a small
    int32 ancestry table ``row_map[r][j]`` names the cache row that holds position j of logical row r, and ``reorder`` permutes it."""

    def __init__(self, gpt2: Gpt2Engine, rows: int, ctx_max: int):
        _require_cuda(gpt2.arena.w32, "DecodeSession")
        self.g = gpt2
        self.R = rows
        self.ctx_max = min(ctx_max, gpt2.dims["NPOS"])
        self.pos = 0
        d = gpt2.dims
        dev = gpt2.arena.device
        # 16-bit operand type; fp32 in the bf16x3 mode (include/clipcap_hip.h OPERAND TYPE)
        self.kv = torch.empty(d["NL"] * 2 * rows * self.ctx_max * d["D"], dtype=torch.float32 if gpt2.op_dtype == OP_X3 else gpt2.arena.w16.dtype,
                              device=dev)
        self.row_map = torch.arange(rows, dtype=torch.int32, device=dev).view(rows, 1).repeat(1, self.ctx_max).contiguous()
        self._ws: Dict[int, torch.Tensor] = {}
        self._logits: Optional[torch.Tensor] = None

    def _workspace(self, tn: int) -> torch.Tensor:
        ws = self._ws.get(tn)
        if ws is None:
            nbytes = _lib.lib().cc_decode_ws_bytes(C.byref(self.g.cfg), self.R, tn)
            check(nbytes, "cc_decode_ws_bytes")
            ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.g.arena.device)     # zeroed: cc_decode_ws_check's error word starts clear
            self._ws[tn] = ws
        return ws

    def forward(self, x: torch.Tensor, rows: Optional[int] = None, partials: bool = False, group: int = 1) -> torch.Tensor:
        """x fp32 (R', Tnew, D) input embeddings (no positional term), R' <= R active rows -> fp32 logits of the last new
        position (R', V).  Valid until the next forward().  ``partials``: also keep the lm_head epilogue's per-64-column softmax
        partials of these logits in ``self.lpart`` = (tensor, npart) for beam_step (cc_decode_fwd_g / cc_beam_step_p).
        ``group``: consecutive rows that share ancestry (beam search: the beam width) — a performance hint, results do not depend on it."""
        g = self.g
        x = x.to(device=g.arena.device, dtype=torch.float32).contiguous()
        Ra, tn, D = x.shape
        assert Ra <= self.R and D == g.dims["D"]
        if self.pos + tn > self.ctx_max:
            raise RuntimeError(f"decode context overflow: {self.pos}+{tn} > {self.ctx_max}")
        g.arena.sync_bf16()
        Vp = g.dims["Vp"]
        if self._logits is None:
            self._logits = torch.empty(self.R, Vp, dtype=torch.float32, device=g.arena.device)
        logits = self._logits[:Ra]
        if Ra != self.R:   # fewer active rows (prefill with one row per sample): the cache row stride is still R rows
            raise RuntimeError("partial-row forward is expressed through a narrower session; use expand()")
        self.lpart = None
        if partials:
            if getattr(self, "_lpart", None) is None:
                n = _lib.lib().cc_decode_part_floats(C.byref(g.cfg), self.R)
                check(n, "cc_decode_part_floats")
                self._lpart = torch.empty(n, dtype=torch.float32, device=g.arena.device)
            self.lpart = (self._lpart, self._lpart.numel() // (2 * self.R))
        grp = int(group) if self.R % max(1, int(group)) == 0 else 1
        wimg, wteam = g.decode_images() if (tn == 1 and _lib.IS_LAB) else (None, None)     # lab library: weight images of the decode experiments
        if wimg is not None or wteam is not None:
            check(_lib.lib().cc_decode_fwd_x(C.byref(g.cfg), Ra, tn, self.pos, self.ctx_max, _p(g.arena.w32), _p(g.arena.w16),
                                            _p(wimg) if wimg is not None else None, _p(wteam) if (wteam is not None and grp >= 2) else None, _p(x), _p(self.kv),
                                            _p(self.row_map), grp, _p(self._workspace(tn)), _p(logits), Vp,
                                            _p(self._lpart) if partials else None, _stream(g.arena.device)), "cc_decode_fwd_x")
        else:
            check(_lib.lib().cc_decode_fwd_g(C.byref(g.cfg), Ra, tn, self.pos, self.ctx_max, _p(g.arena.w32), _p(g.arena.w16), _p(x), _p(self.kv),
                                            _p(self.row_map), grp, _p(self._workspace(tn)), _p(logits), Vp,
                                            _p(self._lpart) if partials else None, _stream(g.arena.device)), "cc_decode_fwd_g")
        self.pos += tn
        self._last_tn = tn
        return logits[:, : g.dims["V"]]

    def hidden_unit(self, out: torch.Tensor, ld_row: int, ld_pos: int) -> torch.Tensor:
        """The final hidden states of the last forward(), all R * Tnew positions, as fp32 unit vectors (cc_decode_hidden_unit; contrastive
        search): out[r * ld_row + t * ld_pos : + D] = ln_f(residual) / its L2 norm, from the fp32 residual stream the forward left in its
        workspace — not from the 16-bit rows the lm_head reads, so the operand mode enters only through the residual itself.  ``out``: a
        contiguous fp32 device tensor that covers those elements (strides in floats, multiples of 4; ld_pos >= D).  Valid until the
        next forward() of this session; RuntimeError before the first one and while the lab library's persistent decode engines are on
        (they keep the residual stream elsewhere).  Returns ``out``."""
        tn = getattr(self, "_last_tn", None)
        if tn is None:
            raise RuntimeError("hidden_unit() needs a forward() on this session first")
        if _lib.lib().cc_decode_mode(-1) & 6:
            raise RuntimeError("hidden_unit() does not support the persistent decode engines (cc_decode_mode bits 1 and 2)")
        g = self.g
        D = g.dims["D"]
        assert out.dtype == torch.float32 and out.is_contiguous() and out.device == g.arena.w32.device
        assert out.numel() >= (self.R - 1) * ld_row + (tn - 1) * ld_pos + D
        check(_lib.lib().cc_decode_hidden_unit(C.byref(g.cfg), self.R, tn, _p(g.arena.w32), _p(self._ws[tn]), _p(out), int(ld_row), int(ld_pos),
                                              _stream(g.arena.device)), "cc_decode_hidden_unit")
        return out

    def check(self, tn: int = 1) -> None:
        """Lab library: synchronises and raises if the last single-position step on this session's workspace gave up on an in-launch
        hand-off of the persistent-launch experiments (cc_decode_ws_check).  The product path has no in-launch hand-offs: nothing to check."""
        if _lib.IS_LAB and tn in self._ws:
            check(_lib.lib().cc_decode_ws_check(C.byref(self.g.cfg), self.R, tn, _p(self._ws[tn]), _stream(self.g.arena.device)), "cc_decode_ws_check")

    def reorder(self, src_rows: torch.Tensor) -> "DecodeSession":
        """Logical row r continues the history of logical row src_rows[r] (same row count): permutes the ancestry table in place."""
        src = src_rows.to(device=self.g.arena.device, dtype=torch.int64)
        if self.pos > 0:
            self.row_map[:, : self.pos] = self.row_map.index_select(0, src)[:, : self.pos]
        return self

    def beam_advance(self, beam: int, next_tok: torch.Tensor, src_local: Optional[torch.Tensor], wte: torch.Tensor, step: int,
                     tokens_in: torch.Tensor, tokens_out: torch.Tensor, x_out: torch.Tensor) -> None:
        """Everything between two beam steps in one launch (cc_beam_advance; reference inference/base.py:104-117): row r continues row
        (r // beam) * beam + src_local[r] (None: itself) — the ancestry table is permuted (into a second buffer, then swapped),
        tokens_out[r] = tokens_in[that row][:step] + [next_tok[r]] (int32 (R, n) buffers) and x_out (R, 1, D) fp32 = wte[next_tok]."""
        if getattr(self, "_row_map_alt", None) is None:
            self._row_map_alt = torch.empty_like(self.row_map)
        check(_lib.lib().cc_beam_advance(C.byref(self.g.cfg), self.R, beam, _p(wte), _p(next_tok), _p(src_local) if src_local is not None else None,
                                        self.pos, self.ctx_max, _p(self.row_map), _p(self._row_map_alt), step, tokens_out.stride(0),
                                        _p(tokens_in), _p(tokens_out), _p(x_out), _stream(self.g.arena.device)), "cc_beam_advance")
        self.row_map, self._row_map_alt = self._row_map_alt, self.row_map

    def expand(self, src_rows: torch.Tensor, rows_out: int) -> "DecodeSession":
        """A wider session (rows_out rows) whose row r starts from this session's row src_rows[r] (beam fan-out after the prefill,
        base.py:93).  The prefix K/V are copied once (cc_decode_reorder)."""
        out = DecodeSession(self.g, rows_out, self.ctx_max)
        out.pos = self.pos
        src = self.row_map[:, 0].index_select(0, src_rows.to(device=self.g.arena.device, dtype=torch.int64)).to(torch.int32).contiguous() \
            if self.pos > 0 else src_rows.to(device=self.g.arena.device, dtype=torch.int32).contiguous()
        check(_lib.lib().cc_decode_reorder(C.byref(self.g.cfg), self.R, rows_out, self.pos, self.ctx_max, _p(self.kv), _p(out.kv), _p(src),
                                          _stream(self.g.arena.device)), "cc_decode_reorder")
        if self.pos > 0:
            # rows fanned out from one source hold identical prefix K / V: their ancestry tables all name the FIRST copy, so that the
            # beam-group attention step (cc_decode_fwd_g) reads one copy per group instead of one per row
            idx = torch.arange(rows_out, dtype=torch.int32, device=src.device)
            first = torch.full((int(self.R),), rows_out, dtype=torch.int32, device=src.device).scatter_reduce(0, src.to(torch.int64), idx, "amin")
            out.row_map[:, : self.pos] = first.index_select(0, src.to(torch.int64)).view(rows_out, 1)
        return out


def embed_tokens(gpt2: "Gpt2Engine", tokens: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out fp32 (R, 1, D) or (R, D) = wte[tokens] for int32 ``tokens`` (R,) in one launch (cc_embed_tokens; reference inference/base.py:117,184)."""
    wte = gpt2.arena.w32[gpt2.offsets[0]:]
    check(_lib.lib().cc_embed_tokens(C.byref(gpt2.cfg), tokens.numel(), _p(wte), _p(tokens), _p(out), _stream(gpt2.arena.device)), "cc_embed_tokens")
    return out


def embed_tokens_bwd(gpt2: "Gpt2Engine", tokens: torch.Tensor, dout: torch.Tensor) -> torch.Tensor:
    """fp32 (V, D) gradient of ``embed_tokens`` with respect to wte: rows of ``dout`` (R, D) scattered by int32 ``tokens`` (R,), rows that
    share an id accumulate in a fixed order, so the result is the same bit for bit from run to run (cc_embed_tokens_bwd_ws; no atomics).
    Its index scratch is kept on the engine and grown when a larger R arrives."""
    D, V, Vp = gpt2.dims["D"], gpt2.dims["V"], gpt2.dims["Vp"]
    L = _lib.lib()
    R = tokens.numel()
    dw = torch.zeros(Vp, D, dtype=torch.float32, device=gpt2.arena.device)
    if R == 0:
        return dw[:V]
    need = L.cc_embed_tokens_bwd_ws_bytes(C.byref(gpt2.cfg), R)
    check(need, "cc_embed_tokens_bwd_ws_bytes")
    ws = getattr(gpt2, "_embed_bwd_ws", None)
    if ws is None or ws.numel() < need or ws.device != dw.device:
        ws = gpt2._embed_bwd_ws = torch.empty(need, dtype=torch.uint8, device=dw.device)
    check(L.cc_embed_tokens_bwd_ws(C.byref(gpt2.cfg), R, _p(dout), _p(tokens), _p(dw), _p(ws), _stream(gpt2.arena.device)), "cc_embed_tokens_bwd_ws")
    return dw[:V]


def beam_buffers(device, samples: int, beam: int, V: int) -> tuple:
    """(next_tokens int32 (samples*beam,), src_rows int32 (samples*beam,), scratch) of cc_beam_step.  Owned by ONE decode (a
    generate_beam_tokens call allocates them once and reuses them from step to step: each step's outputs are consumed by
    cc_beam_advance before the next update) — never shared between decodes, streams or threads."""
    return (torch.empty(samples * beam, dtype=torch.int32, device=device), torch.empty(samples * beam, dtype=torch.int32, device=device),
            torch.empty(_lib.lib().cc_beam_ws_bytes(samples, beam, V), dtype=torch.uint8, device=device))


def beam_step(logits: torch.Tensor, samples: int, beam: int, temperature: float, first: bool, stop_token: int, scores: torch.Tensor,
              seq_lengths: torch.Tensor, has_stopped: torch.Tensor, bufs: Optional[tuple] = None, lpart: Optional[tuple] = None):
    """One device-side beam update for `samples` independent beam sets (reference inference/base.py:84-119).
    logits fp32 (samples*beam, V) (a view with row stride ldl is fine); state tensors are updated IN PLACE.
    ``bufs``: the caller's beam_buffers(...) (fresh ones are allocated when omitted).  ``lpart``: DecodeSession.lpart of the forward
    that produced these logits (softmax partials from the lm_head epilogue): the update then runs as one launch (cc_beam_step_p).
    Returns (next_tokens int32 (samples*beam,), src_rows int32 (samples*beam,) local row index inside each sample)."""
    dev = logits.device
    V = logits.shape[1]
    ldl = logits.stride(0)
    nt, sr, ws = bufs if bufs is not None else beam_buffers(dev, samples, beam, V)
    check(_lib.lib().cc_beam_step_p(samples, beam, V, _p(logits), ldl, _p(lpart[0]) if lpart is not None else None,
                                   lpart[1] if lpart is not None else 0, float(temperature), int(first), int(stop_token), _p(scores),
                                   _p(seq_lengths), _p(has_stopped), _p(nt), _p(sr), _p(ws), _stream(dev)), "cc_beam_step_p")
    return nt, sr


def beam_group_buffers(device, samples: int, beam: int, groups: int, V: int) -> tuple:
    """beam_buffers for beam_group_step: (next_tokens, src_rows, scratch of cc_beam_group_ws_bytes).  Owned by ONE decode, like those."""
    nbytes = _lib.lib().cc_beam_group_ws_bytes(samples, beam, groups, V)
    check(nbytes, "cc_beam_group_ws_bytes")
    return (torch.empty(samples * beam, dtype=torch.int32, device=device), torch.empty(samples * beam, dtype=torch.int32, device=device),
            torch.empty(nbytes, dtype=torch.uint8, device=device))


def beam_group_step(logits: torch.Tensor, samples: int, beam: int, groups: int, temperature: float, diversity_penalty: float, first: bool,
                    stop_token: int, scores: torch.Tensor, seq_lengths: torch.Tensor, has_stopped: torch.Tensor, bufs: Optional[tuple] = None):
    """One device-side update of diverse beam search (cc_beam_group_step; Vijayakumar et al., 2016): the ``beam`` rows of every sample are
    ``groups`` beam groups of beam // groups consecutive rows, advanced one after the other; a token that earlier beam groups picked at
    this step c times loses ``diversity_penalty`` * c of its log-probability in the later ones.  Arguments, in-place state and the result
    (next_tokens, src_rows — the source row inside the sample) are beam_step's; ``bufs``: the caller's beam_group_buffers(...).
    groups == 1 is beam_step without partials, bit for bit."""
    dev = logits.device
    V = logits.shape[1]
    nt, sr, ws = bufs if bufs is not None else beam_group_buffers(dev, samples, beam, groups, V)
    check(_lib.lib().cc_beam_group_step(samples, beam, groups, V, _p(logits), logits.stride(0), float(temperature), float(diversity_penalty),
                                       int(first), int(stop_token), _p(scores), _p(seq_lengths), _p(has_stopped), _p(nt), _p(sr), _p(ws),
                                       _stream(dev)), "cc_beam_group_step")
    return nt, sr


def beam_gumbel_buffers(device, samples: int, beam: int, V: int) -> tuple:
    """beam_buffers for beam_gumbel_step: (next_tokens, src_rows, scratch of cc_beam_gumbel_ws_bytes).  Owned by ONE decode, like those."""
    nbytes = _lib.lib().cc_beam_gumbel_ws_bytes(samples, beam, V)
    check(nbytes, "cc_beam_gumbel_ws_bytes")
    return (torch.empty(samples * beam, dtype=torch.int32, device=device), torch.empty(samples * beam, dtype=torch.int32, device=device),
            torch.empty(nbytes, dtype=torch.uint8, device=device))


def beam_gumbel_step(logits: torch.Tensor, samples: int, beam: int, temperature: float, first: bool, stop_token: int, seed: int, step: int,
                     scores: torch.Tensor, gumbels: torch.Tensor, seq_lengths: torch.Tensor, has_stopped: torch.Tensor,
                     bufs: Optional[tuple] = None):
    """One device-side update of stochastic beam search (cc_beam_gumbel_step; Kool et al., 2019): every sample's ``beam`` slots become
    ``beam`` continuations sampled without replacement from the model, best perturbed log-probability first.  logits fp32 (samples*beam, V)
    (a view with a row stride is fine; ``first``: only row 0 of every sample is read).  State IN PLACE, fp32 (samples*beam,): ``scores`` =
    the summed token log-probabilities (not length-normalised), ``gumbels`` = the perturbed log-probabilities; ``seq_lengths`` and
    ``has_stopped`` (uint8) as beam_step's.  The Gumbel noise is a pure function of (``seed`` in [0, 2^64), ``step`` >= 0, the logits row's
    index, the token): counter-based, drawn inside the kernel.  ``bufs``: the caller's beam_gumbel_buffers(...).
    Returns (next_tokens int32 (samples*beam,), src_rows int32 (samples*beam,) — the source row inside the sample)."""
    dev = logits.device
    V = logits.shape[1]
    nt, sr, ws = bufs if bufs is not None else beam_gumbel_buffers(dev, samples, beam, V)
    ldl = logits.stride(0) if logits.shape[0] > 1 else max(logits.stride(0), V)
    check(_lib.lib().cc_beam_gumbel_step(samples, beam, V, _p(logits), ldl, float(temperature), int(first), int(stop_token), int(seed), int(step),
                                        _p(scores), _p(gumbels), _p(seq_lengths), _p(has_stopped), _p(nt), _p(sr), _p(ws), _stream(dev)),
          "cc_beam_gumbel_step")
    return nt, sr


def beam_lex_buffers(device, samples: int, beam: int, n_phr: int, V: int) -> tuple:
    """beam_buffers for beam_lex_step: (next_tokens, src_rows, scratch of cc_beam_lex_ws_bytes).  Owned by ONE decode, like those."""
    nbytes = _lib.lib().cc_beam_lex_ws_bytes(samples, beam, n_phr, V)
    check(nbytes, "cc_beam_lex_ws_bytes")
    return (torch.empty(samples * beam, dtype=torch.int32, device=device), torch.empty(samples * beam, dtype=torch.int32, device=device),
            torch.empty(nbytes, dtype=torch.uint8, device=device))


def beam_lex_step(logits: torch.Tensor, samples: int, beam: int, temperature: float, first: bool, stop_token: int, scores: torch.Tensor,
                  seq_lengths: torch.Tensor, has_stopped: torch.Tensor, lex_state: torch.Tensor, phrases: Optional[torch.Tensor],
                  bufs: Optional[tuple] = None):
    """One device-side update of lexically constrained beam search (cc_beam_lex_step; dynamic beam allocation, Post & Vilar, 2018): a beam
    may stop only after it has produced every phrase of its sample, and the ``beam`` slots are divided between the candidates by the number
    of constraint tokens they have met, slot 0 the most.  logits fp32 (samples*beam, V) (a view with a row stride is fine; ``first``: only
    row 0 of every sample is read).  ``phrases``: int32 (samples, n_phr, phr_len) on the device, -1 after a phrase's last token, at most 8
    phrases of at most 8 tokens, or None for no phrases (then this is beam_step without partials, bit for bit).  State IN PLACE:
    ``scores``, ``seq_lengths``, ``has_stopped`` as beam_step's and ``lex_state`` int32 (samples*beam,), zeros before the first step (what
    it holds: inference/utils.py unpack_lex_state).  ``bufs``: the caller's beam_lex_buffers(...).
    Returns (next_tokens int32 (samples*beam,), src_rows int32 (samples*beam,) — the source row inside the sample)."""
    dev = logits.device
    V = logits.shape[1]
    n_phr, phr_len = (0, 1) if phrases is None else (int(phrases.shape[1]), int(phrases.shape[2]))
    if phrases is not None and (phrases.dtype != torch.int32 or phrases.dim() != 3 or phrases.shape[0] != samples or not phrases.is_contiguous()):
        raise ValueError(f"phrases must be a contiguous int32 tensor ({samples}, n_phr, phr_len), got {phrases.dtype} {tuple(phrases.shape)}")
    nt, sr, ws = bufs if bufs is not None else beam_lex_buffers(dev, samples, beam, n_phr, V)
    ldl = logits.stride(0) if logits.shape[0] > 1 else max(logits.stride(0), V)
    check(_lib.lib().cc_beam_lex_step(samples, beam, V, _p(logits), ldl, float(temperature), int(first), int(stop_token),
                                     _p(phrases) if n_phr > 0 else None, n_phr, phr_len, _p(scores), _p(seq_lengths), _p(has_stopped),
                                     _p(lex_state), _p(nt), _p(sr), _p(ws), _stream(dev)), "cc_beam_lex_step")
    return nt, sr


def constrain_logits(logits: torch.Tensor, *, lpart: Optional[tuple] = None, history: Optional[torch.Tensor] = None, hist_len: int = 0,
                     no_repeat_ngram: int = 0, ban_token: int = -1, suppress: Optional[torch.Tensor] = None,
                     skip_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Token bans on one step's fp32 ``logits`` (R, V), IN PLACE, before beam_step / sample_step (cc_logits_constrain): a banned token's
    logit becomes -inf, i.e. it is removed before the softmax.  Banned in row r: what repeating would complete an n-gram of size
    ``no_repeat_ngram`` in ``history[r, :hist_len]`` (int32 or int64 (R, >= hist_len), oldest first; inference.utils.banned_tokens states
    the rule), ``ban_token`` (-1: none) and every id of ``suppress`` (int32 device tensor).  Rows with a non-zero ``skip_rows`` entry (uint8
    (R,), e.g. has_stopped) are left alone.  ``lpart``: DecodeSession.lpart of the forward that produced these logits — the partials of the
    64-column blocks that received a ban are recomputed, so that beam_step(..., lpart) stays exact.  A view with a row stride is fine.
    Returns ``logits``."""
    dev = logits.device
    R, V = logits.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    he = 4
    if history is not None:
        assert history.dtype in (torch.int32, torch.int64) and history.shape[0] == R and history.stride(1) == 1
        he = history.element_size()
    if suppress is not None:
        assert suppress.dtype == torch.int32 and suppress.is_contiguous()
    if skip_rows is not None:
        assert skip_rows.dtype == torch.uint8 and skip_rows.numel() == R and skip_rows.is_contiguous()
    check(_lib.lib().cc_logits_constrain(_p(logits), R, V, logits.stride(0), _p(lpart[0]) if lpart is not None else None,
                                        lpart[1] if lpart is not None else 0, _p(history) if history is not None else None, he,
                                        history.stride(0) if history is not None else 0, int(hist_len), int(no_repeat_ngram), int(ban_token),
                                        _p(suppress) if suppress is not None else None, suppress.numel() if suppress is not None else 0,
                                        _p(skip_rows) if skip_rows is not None else None, _stream(dev)), "cc_logits_constrain")
    return logits


def guide_logits(cond: torch.Tensor, uncond: torch.Tensor, scale: float, *, out: Optional[torch.Tensor] = None,
                 skip_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Classifier-free guidance on one step's logits, before the bans and beam_step / sample_step (cc_logits_guide, one launch):
    out = log_softmax(uncond) + scale * (log_softmax(cond) - log_softmax(uncond)) for fp32 ``cond`` / ``uncond`` (R, V), the logits of the
    stream that saw the prefix and of the one that did not.  An entry that is -inf in either input is -inf in the result.  ``out`` None:
    IN PLACE on ``cond``; otherwise an fp32 (R, V) tensor.  Rows with a non-zero ``skip_rows`` entry (uint8 (R,), e.g. has_stopped) are not
    written.  Views with a row stride are fine for all three (decode logits, the first beam step's lg[::beam]).  Returns the tensor written."""
    dev = cond.device
    R, V = cond.shape
    dst = cond if out is None else out
    for t in (cond, uncond, dst):
        assert t.dtype == torch.float32 and t.dim() == 2 and tuple(t.shape) == (R, V) and t.device == dev
        assert V == 1 or t.stride(1) == 1
    if skip_rows is not None:
        assert skip_rows.dtype == torch.uint8 and skip_rows.numel() == R and skip_rows.is_contiguous() and skip_rows.device == dev
    ld = lambda t: t.stride(0) if R > 1 else max(t.stride(0), V)  # noqa: E731   (a one-row view may report any row stride)
    check(_lib.lib().cc_logits_guide(_p(cond), ld(cond), _p(uncond), ld(uncond), R, V, float(scale), _p(dst), ld(dst),
                                    _p(skip_rows) if skip_rows is not None else None, _stream(dev)), "cc_logits_guide")
    return dst


def truncate_logits(logits: torch.Tensor, *, temperature: float = 1.0, history: Optional[torch.Tensor] = None, hist_len: int = 0,
                    repetition_penalty: float = 1.0, min_p: float = 0.0, typical_p: float = 1.0, epsilon_cutoff: float = 0.0,
                    eta_cutoff: float = 0.0) -> torch.Tensor:
    """The truncation rules of the sampling decoders on one step's fp32 ``logits`` (R, V), IN PLACE, after the guidance and the bans and
    immediately before sample_step, called with the same ``temperature``, ``history`` (int64 (R, >= hist_len)), ``hist_len`` and
    ``repetition_penalty`` (cc_logits_truncate, one launch): the rules act on the values the sampler draws from.  A token is kept iff every
    rule that is on keeps it — min_p > 0: p >= min_p * p_max; epsilon_cutoff > 0: p >= epsilon; eta_cutoff > 0: p >= min(eta,
    sqrt(eta) * exp(-entropy)); typical_p < 1: the tokens closest in -log p to the entropy whose mass reaches typical_p, ties kept — every
    rule taken against the same incoming distribution (with one rule on, what the corresponding transformers warper keeps; transformers
    renormalises between several, this does not).  An empty intersection keeps the most probable tokens.  The raw logit of a removed token
    becomes -inf, kept ones stay bit-untouched; sample_step then applies its own top-k / top-p to the truncated row, so its mode-0 top_p
    mass is relative to that row.  With all four off (0, 1, 0, 0) nothing is launched.  A view with a row stride is fine.  ValueError for
    an option outside its range (inference.utils.validate_truncation).  Returns ``logits``."""
    from clipcap_amd.inference.utils import truncation_is_on, validate_truncation
    opts = validate_truncation(min_p, typical_p, epsilon_cutoff, eta_cutoff)
    assert logits.dtype == torch.float32 and logits.dim() == 2
    R, V = logits.shape
    assert V >= 1 and (V == 1 or logits.stride(1) == 1)
    hist_len = int(hist_len)
    if hist_len < 0 or (hist_len > 0 and history is None):
        raise ValueError(f"hist_len = {hist_len} needs a history of at least that many columns")
    if history is not None:
        assert history.dtype == torch.int64 and history.dim() == 2 and history.shape[0] == R and history.device == logits.device
        assert history.shape[1] >= hist_len and (history.shape[1] <= 1 or history.stride(1) == 1)
    if not truncation_is_on(opts) or R == 0:
        return logits
    ld = logits.stride(0) if R > 1 else max(logits.stride(0), V)
    hld = 0 if history is None else (history.stride(0) if R > 1 else max(history.stride(0), hist_len))
    check(_lib.lib().cc_logits_truncate(_p(logits), R, V, ld, float(temperature), _p(history) if history is not None else None, hist_len, hld,
                                       float(repetition_penalty), opts["min_p"], opts["typical_p"], opts["epsilon_cutoff"], opts["eta_cutoff"],
                                       _stream(logits.device)), "cc_logits_truncate")
    return logits


CIDER_MAX_LEN, CIDER_MAX_REF_TOKENS, CIDER_TOKEN_LIMIT = 256, 4096, 65535       # cc_cider_score's limits (include/clipcap_hip.h)


def cider_score(cand: torch.Tensor, refs: torch.Tensor, tab_keys: torch.Tensor, tab_idf: torch.Tensor, log_ndocs: float, *,
                sigma: float = 6.0, stop_token: int = 50256, count_stop: bool = False, ref_count: Optional[torch.Tensor] = None,
                cand_group: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CIDEr-D over TOKEN IDS (cc_cider_score, one launch; nothing is read back): ``cand`` int64 (C, n) candidates, each running to its
    first ``stop_token`` (excluded, or included with ``count_stop``; a negative ``stop_token`` = none), else to its first negative id, else
    n; ``refs`` int32 (G, Rmax, Lr), each row ending at its first negative id; image g uses its first ``ref_count[g]`` rows (int32 (G,),
    1..Rmax; None: all).  Candidate c belongs to image ``cand_group[c]`` (int32 (C,)), or c % G when None (C a multiple of G).
    ``tab_keys`` int64 (cap,) / ``tab_idf`` fp32 (cap,): the idf table of ``train.cider.CiderReward.from_corpus`` (the keys' bit
    patterns), cap a power of two; an n-gram it does not hold gets ``log_ndocs``.  A view with a row stride is fine for ``cand``.
    ValueError for anything cc_cider_score would refuse, before a device is touched.  Returns fp32 (C,) scores (``out`` if given)."""
    import math
    if cand.dim() != 2 or cand.dtype != torch.int64:
        raise ValueError(f"cand must be int64 (C, n), got {cand.dtype} {tuple(cand.shape)}")
    if refs.dim() != 3 or refs.dtype != torch.int32 or not refs.is_contiguous():
        raise ValueError(f"refs must be contiguous int32 (G, Rmax, Lr), got {refs.dtype} {tuple(refs.shape)}")
    C_, n = cand.shape
    G, Rmax, Lr = refs.shape
    if G < 1 or Rmax < 1 or Lr < 1:
        raise ValueError(f"refs must hold at least one image, reference and position, got {tuple(refs.shape)}")
    if n > CIDER_MAX_LEN or Lr > CIDER_MAX_LEN or Rmax * Lr > CIDER_MAX_REF_TOKENS:
        raise ValueError(f"cider_score takes candidates and references of at most {CIDER_MAX_LEN} positions and at most "
                         f"{CIDER_MAX_REF_TOKENS} reference positions per image, got n = {n}, Rmax = {Rmax}, Lr = {Lr}")
    stop_token = int(stop_token)
    if stop_token >= CIDER_TOKEN_LIMIT:
        raise ValueError(f"stop_token must be below {CIDER_TOKEN_LIMIT}, got {stop_token}")
    sigma, log_ndocs = float(sigma), float(log_ndocs)
    if not (sigma > 0.0 and math.isfinite(sigma)) or not math.isfinite(log_ndocs):
        raise ValueError(f"sigma must be positive and finite and log_ndocs finite, got {sigma}, {log_ndocs}")
    if (n > 1 and cand.stride(1) != 1) or (C_ > 1 and cand.stride(0) < n):
        raise ValueError("cand rows must be dense and must not overlap")
    cap = tab_keys.numel()
    if tab_keys.dtype != torch.int64 or tab_idf.dtype != torch.float32 or tab_idf.numel() != cap or cap < 1 or cap & (cap - 1) or \
            not tab_keys.is_contiguous() or not tab_idf.is_contiguous():
        raise ValueError("tab_keys int64 / tab_idf fp32 must be contiguous and hold the same power-of-two number of slots")
    if cand_group is None:
        if C_ % G:
            raise ValueError(f"without cand_group the {C_} candidates must be a multiple of the {G} images")
    elif cand_group.dtype != torch.int32 or cand_group.shape != (C_,) or not cand_group.is_contiguous():
        raise ValueError(f"cand_group must be contiguous int32 ({C_},)")
    if ref_count is not None and (ref_count.dtype != torch.int32 or ref_count.shape != (G,) or not ref_count.is_contiguous()):
        raise ValueError(f"ref_count must be contiguous int32 ({G},)")
    if out is None:
        out = torch.empty(C_, dtype=torch.float32, device=cand.device)
    elif out.dtype != torch.float32 or out.shape != (C_,) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous fp32 ({C_},)")
    for t in (refs, tab_keys, tab_idf, ref_count, cand_group, out):
        if t is not None and t.device != cand.device:
            raise ValueError(f"every tensor must be on the candidates' device {cand.device}, got {t.device}")
    if C_ == 0:
        return out
    _require_cuda(cand, "cider_score")
    ld = cand.stride(0) if C_ > 1 else max(cand.stride(0), n)
    check(_lib.lib().cc_cider_score(_p(cand), C_, n, ld, stop_token, 1 if count_stop else 0, _p(cand_group) if cand_group is not None else None,
                                    _p(refs), G, Rmax, Lr, _p(ref_count) if ref_count is not None else None, _p(tab_keys), _p(tab_idf), cap,
                                    log_ndocs, sigma, _p(out), _stream(cand.device)), "cc_cider_score")
    return out


def _caption_metric_shapes(what: str, cand: torch.Tensor, refs: torch.Tensor, ref_count: Optional[torch.Tensor],
                           cand_group: Optional[torch.Tensor]):
    """What cc_bleu_stats and cc_rouge_l would refuse about their common arguments, as ValueError before a device is touched.
    Returns (C, n, G, Rmax, Lr)."""
    if cand.dim() != 2 or cand.dtype != torch.int64:
        raise ValueError(f"cand must be int64 (C, n), got {cand.dtype} {tuple(cand.shape)}")
    if refs.dim() != 3 or refs.dtype != torch.int32 or not refs.is_contiguous():
        raise ValueError(f"refs must be contiguous int32 (G, Rmax, Lr), got {refs.dtype} {tuple(refs.shape)}")
    C_, n = cand.shape
    G, Rmax, Lr = refs.shape
    if G < 1 or Rmax < 1 or Lr < 1:
        raise ValueError(f"refs must hold at least one image, reference and position, got {tuple(refs.shape)}")
    if n > CIDER_MAX_LEN or Lr > CIDER_MAX_LEN or Rmax * Lr > CIDER_MAX_REF_TOKENS:
        raise ValueError(f"{what} takes candidates and references of at most {CIDER_MAX_LEN} positions and at most "
                         f"{CIDER_MAX_REF_TOKENS} reference positions per image, got n = {n}, Rmax = {Rmax}, Lr = {Lr}")
    if (n > 1 and cand.stride(1) != 1) or (C_ > 1 and cand.stride(0) < n):
        raise ValueError("cand rows must be dense and must not overlap")
    if cand_group is None:
        if C_ % G:
            raise ValueError(f"without cand_group the {C_} candidates must be a multiple of the {G} images")
    elif cand_group.dtype != torch.int32 or cand_group.shape != (C_,) or not cand_group.is_contiguous():
        raise ValueError(f"cand_group must be contiguous int32 ({C_},)")
    if ref_count is not None and (ref_count.dtype != torch.int32 or ref_count.shape != (G,) or not ref_count.is_contiguous()):
        raise ValueError(f"ref_count must be contiguous int32 ({G},)")
    for t in (refs, ref_count, cand_group):
        if t is not None and t.device != cand.device:
            raise ValueError(f"every tensor must be on the candidates' device {cand.device}, got {t.device}")
    return C_, n, G, Rmax, Lr


def bleu_stats(cand: torch.Tensor, refs: torch.Tensor, *, stop_token: int = 50256, count_stop: bool = False,
               ref_count: Optional[torch.Tensor] = None, cand_group: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """BLEU-1..4 over word ids (cc_bleu_stats, one launch; nothing is read back): the reference's bleu_scorer.py with option "closest".
    ``cand``, ``refs``, ``ref_count``, ``cand_group``, ``stop_token`` and ``count_stop`` are ``cider_score``'s, except that any id >= 0
    is a word and ``stop_token`` has no upper limit.  Returns (stats int32 (C, 10): L, reflen, guess[1..4], correct[1..4] per candidate,
    exact; bleu fp32 (C, 4): the sentence scores).  ``bleu_corpus(stats)`` gives the corpus score.  ValueError for anything
    cc_bleu_stats would refuse, before a device is touched."""
    C_, n, G, Rmax, Lr = _caption_metric_shapes("bleu_stats", cand, refs, ref_count, cand_group)
    stats = torch.empty(C_, 10, dtype=torch.int32, device=cand.device)
    bleu = torch.empty(C_, 4, dtype=torch.float32, device=cand.device)
    if C_ == 0:
        return stats, bleu
    _require_cuda(cand, "bleu_stats")
    ld = cand.stride(0) if C_ > 1 else max(cand.stride(0), n)
    check(_lib.lib().cc_bleu_stats(_p(cand), C_, n, ld, int(stop_token), 1 if count_stop else 0,
                                   _p(cand_group) if cand_group is not None else None, _p(refs), G, Rmax, Lr,
                                   _p(ref_count) if ref_count is not None else None, _p(stats), _p(bleu), _stream(cand.device)),
          "cc_bleu_stats")
    return stats, bleu


ROUGE_BETA = 1.2                                                                # the reference's rouge.py


def rouge_l(cand: torch.Tensor, refs: torch.Tensor, *, stop_token: int = 50256, count_stop: bool = False,
            ref_count: Optional[torch.Tensor] = None, cand_group: Optional[torch.Tensor] = None,
            beta: float = ROUGE_BETA) -> Tuple[torch.Tensor, torch.Tensor]:
    """ROUGE-L over word ids (cc_rouge_l, one launch; nothing is read back): the reference's rouge.py, except that an empty candidate
    scores 0 and an empty reference adds 0 to both maxima.  Arguments as ``bleu_stats``; ``beta`` is rounded to fp32 on its way to the
    kernel.  Returns (score fp32 (C,), lcs int32 (C, Rmax): the exact LCS length against every reference row in use, -1 for the
    others).  ValueError for anything cc_rouge_l would refuse, before a device is touched."""
    import math
    C_, n, G, Rmax, Lr = _caption_metric_shapes("rouge_l", cand, refs, ref_count, cand_group)
    beta = float(beta)
    if not (beta > 0.0 and math.isfinite(beta)):
        raise ValueError(f"beta must be positive and finite, got {beta}")
    score = torch.empty(C_, dtype=torch.float32, device=cand.device)
    lcs = torch.empty(C_, Rmax, dtype=torch.int32, device=cand.device)
    if C_ == 0:
        return score, lcs
    _require_cuda(cand, "rouge_l")
    ld = cand.stride(0) if C_ > 1 else max(cand.stride(0), n)
    check(_lib.lib().cc_rouge_l(_p(cand), C_, n, ld, int(stop_token), 1 if count_stop else 0,
                                _p(cand_group) if cand_group is not None else None, _p(refs), G, Rmax, Lr,
                                _p(ref_count) if ref_count is not None else None, beta, _p(lcs), _p(score), _stream(cand.device)),
          "cc_rouge_l")
    return score, lcs


def bleu_from_counts(counts) -> List[float]:
    """[BLEU-1 .. BLEU-4] from ten numbers L, reflen, guess[1..4], correct[1..4] — a sentence's, or a corpus's sums — in Python float64,
    as the reference's bleu_scorer.py computes both."""
    import math
    L, reflen, guess, correct = counts[0], counts[1], counts[2:6], counts[6:10]
    tiny, small = 1e-15, 1e-9
    out, p = [], 1.0
    for n in range(4):
        p *= (float(correct[n]) + tiny) / (float(guess[n]) + small)
        out.append(p ** (1.0 / (n + 1)))
    ratio = (L + tiny) / (reflen + small)
    if ratio < 1:
        out = [b * math.exp(1 - 1 / ratio) for b in out]
    return out


def bleu_corpus(stats: torch.Tensor) -> List[float]:
    """The corpus BLEU-1..4 of ``bleu_stats``'s ``stats`` (C, 10): the ten columns are summed on their device in int64, the ten sums read
    back, and the formula runs in Python float64 — exact up to float64, as the integers are exact."""
    if stats.dim() != 2 or stats.shape[1] != 10 or stats.dtype != torch.int32:
        raise ValueError(f"stats must be int32 (C, 10), got {stats.dtype} {tuple(stats.shape)}")
    return bleu_from_counts(stats.sum(dim=0, dtype=torch.int64).tolist())


def contrastive_buffers(device, S: int, k: int, D: int, ctx_max: int, entry_length: int):
    """The device state of ONE contrastive-search decode of S captions with k candidates each (never shared between decodes, streams or
    threads), as a namespace: cand_tok int32 (S*k,), cand_prob fp32 (S*k,), cand_h fp32 (S*k, D) — the candidates of the step;
    hist fp32 (S, ctx_max, D) — the unit hidden states of the context, row j = position j; stopped uint8 (S,), lengths int32 (S,),
    sel int32 (S,), src_rows int32 (S*k,), skip_rows uint8 (S*k,) — contrastive_select's outputs; captions int32 (S, entry_length) and
    scores fp32 (entry_length, S) — token and score of every step (zeros where nothing was generated)."""
    from types import SimpleNamespace
    z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=device)  # noqa: E731
    return SimpleNamespace(cand_tok=z(S * k, dtype=torch.int32), cand_prob=z(S * k, dtype=torch.float32), cand_h=z(S * k, D, dtype=torch.float32),
                           hist=z(S, ctx_max, D, dtype=torch.float32), stopped=z(S, dtype=torch.uint8), lengths=z(S, dtype=torch.int32),
                           sel=z(S, dtype=torch.int32), src_rows=z(S * k, dtype=torch.int32), skip_rows=z(S * k, dtype=torch.uint8),
                           captions=z(S, entry_length, dtype=torch.int32), scores=z(entry_length, S, dtype=torch.float32))


def contrastive_topk(logits: torch.Tensor, S: int, rows_per: int, sel: Optional[torch.Tensor], k: int, stopped: Optional[torch.Tensor],
                     cand_tok: torch.Tensor, cand_prob: torch.Tensor):
    """The k candidates of S captions in one launch (cc_contrastive_topk; Su et al., 2022): caption s reads row s * rows_per + sel[s]
    (``sel`` None: the first) of fp32 ``logits`` (S * rows_per, V) (a view with a row stride is fine).  cand_tok[s*k + c] = the ids of the k
    largest logits, largest first, ties to the lower id; cand_prob[s*k + c] = their softmax probabilities over the whole row (banned,
    -inf, entries contribute nothing).  A slot without a finite logit, and every slot of a caption with a non-zero ``stopped`` entry
    (uint8 (S,), may be None; its row is not read), holds token 0 and probability -1 = invalid.  Returns (cand_tok, cand_prob)."""
    dev = logits.device
    R, V = logits.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and R == S * rows_per
    assert cand_tok.dtype == torch.int32 and cand_prob.dtype == torch.float32 and cand_tok.numel() == S * k == cand_prob.numel()
    assert sel is None or (sel.dtype == torch.int32 and sel.numel() == S)
    assert stopped is None or (stopped.dtype == torch.uint8 and stopped.numel() == S)
    check(_lib.lib().cc_contrastive_topk(_p(logits), logits.stride(0), S, rows_per, _p(sel) if sel is not None else None, V, int(k),
                                        _p(stopped) if stopped is not None else None, _p(cand_tok), _p(cand_prob), _stream(dev)), "cc_contrastive_topk")
    return cand_tok, cand_prob


def contrastive_select(bufs, k: int, hist_lo: int, hist_n: int, alpha: float, stop_token: int, step: int) -> None:
    """One selection step of contrastive search for every caption of ``bufs`` (contrastive_buffers), in one launch
    (cc_contrastive_select): with deg(c) = the largest dot product of candidate c's unit vector bufs.cand_h[s*k + c] with
    bufs.hist[s, hist_lo:hist_n] (0 for an empty range), the slot with the largest (1 - alpha) * cand_prob - alpha * deg among the valid
    ones wins, ties to the lowest slot.  IN PLACE: sel[s] = the winner, captions[s, step] = its token, scores[step, s] = its score,
    hist[s, hist_n] = its vector, lengths[s] += 1, stopped[s] = (token == stop_token), src_rows[s*k + c] = the winner (what beam_advance
    takes), skip_rows[s*k + c] = 1 except on the winner's row of a caption that goes on (what constrain_logits takes).  A caption without a
    valid slot stops with ``stop_token``; one that had stopped before gets padding (token 0, score 0) and keeps its state."""
    S, n, D = bufs.hist.shape
    assert bufs.cand_h.shape == (S * k, D) and bufs.captions.shape[0] == S and bufs.scores.shape[1] == S
    check(_lib.lib().cc_contrastive_select(S, int(k), D, _p(bufs.cand_h), _p(bufs.cand_prob), _p(bufs.cand_tok), _p(bufs.hist), n, int(hist_lo), int(hist_n),
                                          float(alpha), int(stop_token), _p(bufs.stopped), _p(bufs.lengths), _p(bufs.sel), _p(bufs.src_rows),
                                          _p(bufs.skip_rows), _p(bufs.captions), bufs.captions.stride(0), int(step), _p(bufs.scores[step]),
                                          _stream(bufs.hist.device)), "cc_contrastive_select")


def sample_step(logits: torch.Tensor, u: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0, mode: int = 0,
                history: torch.Tensor = None, hist_len: int = 0, repetition_penalty: float = 1.0, return_probs: bool = False,
                length_penalty_stop: int = -1, length_penalty: float = 1.0):
    """One device-side sampling step for every row of fp32 ``logits`` (R, V) (reference inference/base.py:159-184 for mode 0 =
    generate_nucleus_sampling, :245-262 + utils.py:5-37 for mode 1 = top_k_top_p_filtering + softmax).  ``u`` (R,) uniforms in
    [0, 1) drive the inverse-CDF draw; ``history`` int64 (R, >= hist_len) feeds the repetition penalty and, with
    ``length_penalty_stop`` >= 0, the sentence-length penalty of no_beam.py:55-60 (history tokens whose filtered value equals
    float(stop id) are multiplied by ``length_penalty``, utils.py:40-51).
    Returns next_tokens int32 (R,) [, probs fp32 (R, V) — the pre-sampling distribution]."""
    dev = logits.device
    R, V = logits.shape
    nt = torch.empty(R, dtype=torch.int32, device=dev)
    probs = torch.empty(R, V, dtype=torch.float32, device=dev) if return_probs else None
    if history is not None:
        assert history.dtype == torch.int64 and history.shape[0] == R and history.stride(1) == 1
    check(_lib.lib().cc_sample_step_lp(_p(logits), R, V, logits.stride(0), float(temperature), int(top_k or 0), float(top_p or 0.0), int(mode),
                                      _p(history) if history is not None else None, int(hist_len),
                                      history.stride(0) if history is not None else 0, float(repetition_penalty), int(length_penalty_stop),
                                      float(length_penalty), _p(u), _p(nt), _p(probs) if probs is not None else None, _stream(dev)),
          "cc_sample_step_lp")
    return (nt, probs) if return_probs else nt
