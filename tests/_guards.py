"""Guarded, poisoned allocation for the tests that ask WHERE the kernels write and WHAT they read.

``with guarded(fill) as g:`` changes four things while it is active:

* every ``torch.empty`` / ``empty_like`` / ``empty_strided`` / ``zeros`` / ``zeros_like`` / ``full`` on a guarded
  device (CUDA; the host tests pass ``device_types=("cpu",)``) gets a buffer of its own laid out as
  ``[guard | payload | guard]``.  Both guards and the payload of an ``empty*`` call are filled with the byte ``fill``;
  ``zeros`` / ``full`` payloads keep their contract.  The tensor handed back has the requested shape, dtype and strides
  and starts ``GUARD`` bytes (a multiple of 256) into a fresh allocation, so it keeps the alignment the kernels ask for;
  the trailing guard starts at the first byte behind the payload.
* ``ops.workspace`` (and the name ``topk`` imported from it) returns a fresh guarded buffer of EXACTLY ``nbytes``: the
  ``ws_bytes`` that reaches the C ABI is what the size function returned, not the shared scratch of >= 1 MiB.
* the caches of the Python layer that hold device scratch across calls (``ops._WS``, ``_NCE_WS``, ``_SPLIT_CACHE``, ...)
  and the cached answers of the size functions start empty and are put back on exit, so the guarded run allocates and
  sizes everything itself.
* ``lib.raw`` notes what every ``*_workspace_bytes`` function returns (``g.size_values``).
* sealed launch programs (``plan.Programs._seal``) get no floor under their per-stream workspaces (``plan.WS_FLOOR`` = 0):
  each is a guarded buffer of exactly the maximum ``avid_program_workspace_bytes`` reported for that stream.  Every seal
  is noted in ``g.programs`` as (``ws_bytes``, numel of the buffers, bytes passed to the C side, the size function's answers).

``g.place(t)`` copies a test input into a guarded buffer (a read past its end sees the pattern), ``g.check()`` asserts
that every guard byte still holds the pattern and names the buffer (call site inside ``avid-cma_amd/``) and the offset
of the first byte that does not.

The two fills of a test are ``0xFF`` (float NaN, integer -1) and ``0x5A`` (a finite float of about 1.5e16, a large
positive integer): results that are the same bits under both were written in full and depend on nothing unwritten.

The interception is a ``TorchFunctionMode``.  A mode is thread-local and autograd runs CUDA backward nodes on a thread
of its own, so the ``torch`` name that ``ops`` / ``plan`` / ``topk`` / ``parallel`` see is ALSO replaced by a
forwarding proxy whose six factory functions go through the same allocator (a thread-local flag keeps the two from
guarding one allocation twice).  Both stay: the proxy is what is known to reach the backward thread, the mode is what reaches
allocations made outside those four modules (models/, criterions/, the tests' own ``torch.zeros`` for running statistics).  Allocations are counted per call site (``g.sites``, ``g.count_in("backward")``): a
test with a backward asserts that the count there is non-zero.
"""
import contextlib
import os
import sys
import threading

import pytest
import torch
from torch.overrides import TorchFunctionMode

GUARD = 64 * 1024                     # bytes of each guard band: >= 64 KiB, a multiple of 256
FILLS = (0xFF, 0x5A)
_HERE = os.path.abspath(__file__)
_PKG_DIR = os.sep + "avid-cma_amd" + os.sep
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__)) + os.sep

_EMPTY = (torch.empty, torch.empty_like, torch.empty_strided)
_ZEROS = (torch.zeros, torch.zeros_like)
_LIKE = (torch.empty_like, torch.zeros_like)
_FACTORIES = {f: f.__name__ for f in _EMPTY + _ZEROS + (torch.full,)}

_tls = threading.local()


class GuardError(AssertionError):
    pass


class _Record:
    __slots__ = ("buf", "nbytes", "site", "func", "callers", "kind", "thread")

    def __init__(self, buf, nbytes, site, func, callers, kind):
        self.buf, self.nbytes, self.site, self.func, self.callers, self.kind = buf, nbytes, site, func, callers, kind
        self.thread = threading.get_ident()


def _call_site():
    """("file.py:line", function name, names of all calling functions inside avid-cma_amd/): the site is the first frame
    inside avid-cma_amd/, else the first frame that is neither this module nor torch."""
    f = sys._getframe(1)
    first = site = None
    inside = set()
    while f is not None:
        fn = f.f_code.co_filename
        if _PKG_DIR in fn:
            inside.add(f.f_code.co_name)
            if site is None:
                site = (f"{fn[fn.index(_PKG_DIR) + 1:]}:{f.f_lineno}", f.f_code.co_name)
        elif first is None and fn != _HERE and not fn.startswith(_TORCH_DIR) and not fn.startswith("<"):
            first = (f"{os.path.basename(fn)}:{f.f_lineno}", f.f_code.co_name)
        f = f.f_back
    if site is None:
        site = first or ("?", "?")
        inside.add(site[1])
    return site[0], site[1], frozenset(inside)


def _extent(size, stride):
    """Elements of storage a tensor of this size and stride spans (0 for an empty tensor)."""
    if any(s == 0 for s in size):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(size, stride))


class Guards:
    def __init__(self, fill, device_types=("cuda",)):
        assert 0 <= fill <= 255 and GUARD % 256 == 0 and GUARD >= 64 * 1024
        self.fill = int(fill)
        self.device_types = tuple(device_types)
        self.records = []
        self.sites = {}               # (site, function) -> allocations
        self.workspaces = []          # (nbytes asked for, site, names of the calling functions inside avid-cma_amd/)
        self.programs = []            # per sealed program: (ws_bytes [4], buffer numel [4], bytes given to the C side [4], size answers [[4], ...])
        self._needs = []
        self.size_values = set()      # what the *_workspace_bytes functions returned while guarded
        self._lock = threading.Lock()
        self._main = threading.get_ident()

    # ---- allocation ----------------------------------------------------------------------------------------
    def _guarded(self, device):
        return torch.device(device).type in self.device_types

    def raw(self, nbytes, device, kind, payload="fill", value=None, dtype=torch.uint8, size=None, stride=None):
        """[guard | payload of nbytes | guard]; returns the payload viewed as (dtype, size, stride)."""
        site, func, callers = _call_site()
        nbytes = int(nbytes)
        total = -(-(2 * GUARD + nbytes) // 256) * 256
        prev, _tls.inside = getattr(_tls, "inside", False), True
        try:
            buf = torch.empty(total, dtype=torch.uint8, device=device)
            buf.fill_(self.fill)
            flat = buf[GUARD:GUARD + nbytes].view(dtype)
            t = flat if size is None else flat.as_strided(tuple(size), tuple(stride))
            if payload == "zeros":
                flat.zero_()
            elif payload == "full":
                flat.fill_(value)
        finally:
            _tls.inside = prev
        with self._lock:
            self.records.append(_Record(buf, nbytes, site, func, callers, kind))
            self.sites[(site, func)] = self.sites.get((site, func), 0) + 1
        return t

    def factory(self, func, args, kwargs):
        """One of the six factory functions; NotImplemented if the result is not for a guarded device."""
        kwargs = dict(kwargs or {})
        device = kwargs.get("device")
        if device is None:
            device = args[0].device if func in _LIKE else torch.get_default_device()
        if not self._guarded(device):
            return NotImplemented
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        meta_kwargs = {k: v for k, v in kwargs.items() if k not in ("pin_memory", "requires_grad", "out")}
        meta_kwargs["device"] = "meta"
        prev, _tls.inside = getattr(_tls, "inside", False), True
        try:
            meta = func(*args, **meta_kwargs)
        finally:
            _tls.inside = prev
        size, stride, dtype = tuple(meta.shape), tuple(meta.stride()), meta.dtype
        nbytes = _extent(size, stride) * meta.element_size()
        if func in _ZEROS:
            t = self.raw(nbytes, device, _FACTORIES[func], "zeros", None, dtype, size, stride)
        elif func is torch.full:
            value = args[1] if len(args) > 1 else kwargs["fill_value"]
            t = self.raw(nbytes, device, "full", "full", value, dtype, size, stride)
        else:
            t = self.raw(nbytes, device, _FACTORIES[func], "fill", None, dtype, size, stride)
        if kwargs.get("requires_grad"):
            t.requires_grad_(True)
        return t

    def workspace(self, device, nbytes):
        """The stand-in of ``ops.workspace``: exactly ``nbytes``, guarded, poisoned."""
        t = self.raw(int(nbytes), device, "workspace")
        assert t.numel() == int(nbytes)
        self.workspaces.append((int(nbytes), self.records[-1].site, self.records[-1].callers))
        return t

    def place(self, t):
        """A copy of ``t`` (same shape, strides, dtype, requires_grad) in a guarded buffer.  None stays None."""
        if t is None:
            return None
        src = t.detach()
        size, stride = tuple(src.shape), tuple(src.stride())
        out = self.raw(_extent(size, stride) * src.element_size(), src.device, "input", "fill", None, src.dtype, size, stride)
        out.copy_(src)
        if t.requires_grad:
            out.requires_grad_(True)
        return out

    # ---- bookkeeping ---------------------------------------------------------------------------------------
    def count_in(self, function):
        """Allocations made by, or below, a function of avid-cma_amd/ called ``function`` (e.g. "backward")."""
        return sum(1 for r in self.records if function in r.callers)

    def count_off_thread(self):
        return sum(1 for r in self.records if r.thread != self._main)

    def check(self):
        """Every guard byte still holds the pattern, or GuardError naming buffer, band and offset."""
        if any(r.buf.is_cuda for r in self.records):
            torch.cuda.synchronize()
        prev, _tls.inside = getattr(_tls, "inside", False), True
        try:
            with torch.no_grad():
                bad = {}                                  # device -> counts of changed guard bytes, one per record there
                for r in self.records:
                    lead, trail = r.buf[:GUARD], r.buf[GUARD + r.nbytes:]
                    bad.setdefault(r.buf.device, []).append((lead != self.fill).sum() + (trail != self.fill).sum())
                per_dev = {d: iter(torch.stack(v).cpu().tolist()) for d, v in bad.items()}     # one synchronisation per device
                counts = [next(per_dev[r.buf.device]) for r in self.records]
                msgs = []
                for r, n in zip(self.records, counts):
                    if not n:
                        continue
                    for name, band, base in (("leading", r.buf[:GUARD], -GUARD), ("trailing", r.buf[GUARD + r.nbytes:], r.nbytes)):
                        hit = (band != self.fill).nonzero().flatten().cpu()
                        if hit.numel():
                            first, last = int(hit[0]), int(hit[-1])
                            where = (f"{GUARD - first} bytes before the payload" if name == "leading"
                                     else f"{first} bytes past the end of the payload")
                            msgs.append(f"{r.kind} buffer of {r.nbytes} bytes from {r.site} ({r.func}): {hit.numel()} bytes of "
                                        f"the {name} guard overwritten, first at payload offset {base + first} ({where}), "
                                        f"last at {base + last}; fill 0x{self.fill:02X}, first byte now "
                                        f"0x{int(band[first]):02X}")
        finally:
            _tls.inside = prev
        if msgs:
            raise GuardError("guard bytes overwritten:\n  " + "\n  ".join(msgs))


class _Mode(TorchFunctionMode):
    def __init__(self, g):
        super().__init__()
        self.g = g

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func in _FACTORIES and not getattr(_tls, "inside", False):
            out = self.g.factory(func, args, kwargs)
            if out is not NotImplemented:
                return out
        return func(*args, **kwargs)


class _TorchProxy:
    """Stands in for the module-level name ``torch`` of a module: everything forwards to torch, except that the six
    factory functions go through the guarded allocator whichever thread calls them."""

    def __init__(self, g):
        object.__setattr__(self, "_g", g)
        for f, name in _FACTORIES.items():
            object.__setattr__(self, name, self._wrap(f))

    def _wrap(self, f):
        g = self._g

        def factory(*args, **kwargs):
            if not getattr(_tls, "inside", False):
                out = g.factory(f, args, kwargs)
                if out is not NotImplemented:
                    return out
            return f(*args, **kwargs)
        factory.__name__ = f.__name__
        return factory

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        setattr(torch, name, value)


# caches of the Python layer that keep device scratch, or a size function's answer, across calls
_CACHES = {"ops": ("_WS", "_SPLIT_CACHE", "_NCE_WS", "_LOGSPEC_BASIS", "_DESC_CACHE", "_BN_WS_CACHE", "_GROUP_WS_BYTES")}


@contextlib.contextmanager
def guarded(fill, device_types=("cuda",), package=True):
    """See the module docstring.  ``package=False`` (the host tests): only the allocation mode, avid_hip is not imported."""
    g = Guards(fill, device_types)
    with pytest.MonkeyPatch.context() as mp:
        saved = []
        if package:
            from avid_hip import lib, ops, parallel, plan, topk
            mods = {"ops": ops, "plan": plan, "topk": topk, "parallel": parallel}
            mp.setattr(ops, "workspace", g.workspace)
            mp.setattr(topk, "workspace", g.workspace)
            proxy = _TorchProxy(g)
            for m in mods.values():
                mp.setattr(m, "torch", proxy)
            real_raw = lib.raw

            def raw(name):
                fn = real_raw(name)
                if not name.endswith("_workspace_bytes") or name == "avid_program_workspace_bytes":
                    return fn

                def sized(*a):
                    n = fn(*a)
                    g.size_values.add(int(n))
                    return n
                return sized
            mp.setattr(lib, "raw", raw)
            real_call = lib.call

            def call(name, *args):
                real_call(name, *args)
                if name == "avid_program_workspace_bytes":       # (prog, begin, end, n_streams, out_bytes[n_streams])
                    g._needs.append([int(v) for v in args[4]])
            mp.setattr(lib, "call", call)
            mp.setattr(plan, "WS_FLOOR", 0)
            real_seal = plan.Programs._seal

            def seal(self, b, *programs):
                first = len(g._needs)
                progs = real_seal(self, b, *programs)
                g.programs.append((list(self.ws_bytes), [t.numel() for t in self.ws], [self.ws_arr[k].bytes for k in range(4)],
                                   g._needs[first:]))
                return progs
            mp.setattr(plan.Programs, "_seal", seal)
            for mod, names in _CACHES.items():
                for name in names:
                    d = getattr(mods[mod], name)
                    saved.append((d, dict(d)))
                    d.clear()
            inst = ops.DeviceErrors._inst
            saved.append((inst, dict(inst)))
            inst.clear()
        try:
            with _Mode(g):
                yield g
        finally:
            for d, old in saved:
                d.clear()
                d.update(old)
