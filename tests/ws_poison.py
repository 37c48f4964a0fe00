"""Framed, pre-filled buffers to put in place of the engines' cached workspaces (tests/test_gpu_workspace_poison.py).

The library's contract ("What a workspace may hold"): a workspace may hold anything on entry, a call reads only what its own
chain wrote, and nothing is written outside the bytes ``cc_*_ws_bytes`` promised.  A ``Framed`` buffer makes both halves checkable: its
body is filled with one byte before the first call (zeros for run A, 0xFF for run B — NaN in every float type the kernels use, -1 as an
int32) and sits between two guards that must survive.  ``inject`` places the body where an engine keeps its cached buffer, so that the
engine finds it instead of allocating one; ``Injection.verify`` then proves that the engine still holds exactly that buffer.

No GPU code of its own: everything here runs on ``device="cpu"`` too (tests/test_ws_poison.py)."""
import contextlib
import ctypes as C

import torch

GUARD = 4096
GUARD_BYTE = 0xA5
ALIGN = 256
FILL_ZERO = 0x00
FILL_NAN = 0xFF        # fp32 / bf16 / fp16: a NaN; int32: -1, which ce_targets and embed_concat already clamp as a pad id
FILLS = (FILL_ZERO, FILL_NAN)      # no other pattern: in particular none that reads as a large positive integer


class Framed:
    """One uint8 tensor ``buf`` = [GUARD bytes of 0xA5 | body of nbytes, every byte ``fill`` | GUARD bytes of 0xA5]; ``body`` starts on a
    256-byte boundary, like every buffer the carvers hand out."""

    def __init__(self, nbytes: int, fill: int, device):
        assert fill in FILLS, f"fill must be FILL_ZERO or FILL_NAN, got {fill:#x}"
        assert nbytes >= 1
        self.nbytes, self.fill = int(nbytes), int(fill)
        raw = torch.empty(self.nbytes + 2 * GUARD + ALIGN, dtype=torch.uint8, device=device)
        skip = (-raw.data_ptr()) % ALIGN             # GUARD is a multiple of ALIGN: aligning the frame aligns the body
        self.buf = raw[skip:skip + self.nbytes + 2 * GUARD]
        self.lo, self.body, self.hi = self.buf[:GUARD], self.buf[GUARD:GUARD + self.nbytes], self.buf[GUARD + self.nbytes:]
        self.lo.fill_(GUARD_BYTE)
        self.hi.fill_(GUARD_BYTE)
        self.body.fill_(self.fill)
        assert self.body.data_ptr() % ALIGN == 0 and self.body.numel() == self.nbytes and self.hi.numel() == GUARD

    def refill(self, fill=None) -> None:
        """Fill the body again (with another of the two patterns if given); touched() then refers to the new fill."""
        if fill is not None:
            assert fill in FILLS
            self.fill = int(fill)
        self.body.fill_(self.fill)

    def check_guards(self) -> None:
        for name, g in (("below", self.lo), ("above", self.hi)):
            bad = (g != GUARD_BYTE).nonzero()
            assert bad.numel() == 0, f"{bad.numel()} guard bytes {name} the {self.nbytes}-byte body were overwritten, the first at offset " \
                                     f"{int(bad[0]) - GUARD if name == 'below' else self.nbytes + int(bad[0])} of the body"

    def touched(self) -> bool:
        return bool((self.body != self.fill).any())

    def view(self, dtype) -> torch.Tensor:
        """The body as ``dtype`` elements (whole elements only)."""
        n = self.nbytes // torch.empty(0, dtype=dtype).element_size() * torch.empty(0, dtype=dtype).element_size()
        return self.body[:n].view(dtype)


class _Slot:
    def __init__(self, name, framed, get):
        self.name, self.framed, self.get = name, framed, get
        self.ptr = framed.body.data_ptr()


class Injection:
    """The framed buffers placed into a set of engines, and where each sits."""

    def __init__(self):
        self.slots = []

    def add(self, name: str, framed: Framed, get) -> Framed:
        self.slots.append(_Slot(name, framed, get))
        return framed

    def __getitem__(self, name: str) -> Framed:
        return next(s.framed for s in self.slots if s.name == name)

    def verify(self, touched: bool = True) -> None:
        """Every engine still holds the injected tensor (it did not allocate one of its own), no guard byte changed, and (``touched``)
        every body was written to."""
        for s in self.slots:
            cur = s.get()
            assert cur is not None and cur.data_ptr() == s.ptr, f"{s.name}: the engine replaced the injected buffer"
            s.framed.check_guards()
            if touched:
                assert s.framed.touched(), f"{s.name}: no byte of the injected buffer was written — the call did not use it"


def inject(holder, key, framed: Framed, dtype=torch.uint8, injection: Injection = None, name: str = None) -> Framed:
    """Place ``framed.body`` (viewed as ``dtype``) where an engine caches a buffer: ``holder[key]`` for the dicts (MapperEngine._ws,
    Gpt2Engine._ws), ``setattr(holder, key, ...)`` for the attributes (_score_ws, smooth_scratch, _embed_bwd_ws, GradClipper.scratch)."""
    t = framed.view(dtype)
    if isinstance(holder, dict):
        holder[key] = t
        get = lambda: holder.get(key)            # noqa: E731
    else:
        setattr(holder, key, t)
        get = lambda: getattr(holder, key, None)  # noqa: E731
    if injection is not None:
        injection.add(name or str(key), framed, get)
    return framed


@contextlib.contextmanager
def injected_workspaces(specs, fill: int, device="cuda", touched: bool = True):
    """specs: [(name, holder, key, nbytes, dtype)] -> an Injection with one Framed(nbytes, fill) per entry, in place before the body of the
    ``with`` runs; on a clean exit: Injection.verify()."""
    inj = Injection()
    for name, holder, key, nbytes, dtype in specs:
        inject(holder, key, Framed(nbytes, fill, device), dtype, inj, name)
    yield inj
    if device != "cpu":
        torch.cuda.synchronize()
    inj.verify(touched)


# ---- sizes, from the library's own size functions (imported lazily: the module itself needs no library) ----
def _lib():
    from clipcap_amd import _lib as L
    return L.lib(), L.check


def mapper_ws_bytes(me, B: int, save: int) -> int:
    l, check = _lib()
    return check(l.cc_mapper_ws_bytes(C.byref(me.cfg), B, save), "cc_mapper_ws_bytes")


def gpt2_ws_bytes(ge, shp) -> int:
    l, check = _lib()
    return check(l.cc_gpt2_ws_bytes(C.byref(ge.cfg), C.byref(shp)), "cc_gpt2_ws_bytes")


def smooth_scratch_bytes(ge, shp) -> int:
    l, check = _lib()
    return 4 * check(l.cc_lmhead_smooth_scratch_floats(C.byref(ge.cfg), C.byref(shp)), "cc_lmhead_smooth_scratch_floats")


def embed_bwd_ws_bytes(ge, R: int) -> int:
    l, check = _lib()
    return check(l.cc_embed_tokens_bwd_ws_bytes(C.byref(ge.cfg), R), "cc_embed_tokens_bwd_ws_bytes")


def grad_norm_scratch_bytes() -> int:
    l, _ = _lib()
    return 4 * l.cc_grad_norm_scratch_floats()
