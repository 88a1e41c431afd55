"""The one owner of a ``libeioku_hip`` handle, and the one loader of its weights.

Every model class of this package holds a :class:`Handle` (``_h``; the OCR reader ``_d`` and ``_r``) and nothing else
that needs releasing.  The handle creates (``eioku_<prefix>_create``), destroys (``close`` / ``__del__``, the only ones
in the package), refuses to be used once closed, and carries the loaders every ``eioku_<prefix>_*`` family shares:
``convs`` / ``set_convs`` over ``num_convs, conv_info, set_conv``, ``tensors`` / ``set_tensors`` over ``num_tensors,
tensor_info, set_tensor``, and ``doubles`` for the ``last_flops`` / ``last_ms`` getters.
"""
from __future__ import annotations

import ctypes as C
from functools import partial

import numpy as np

from . import _lib
from ._lib import EiokuHipError

_NAME = 256  # bytes for a layer or tensor name


class Handle:
    """``Handle("yolo", ch, depth, nc)``: ``eioku_yolo_create(ch, depth, nc, &h)`` now, ``eioku_yolo_destroy(h)`` at
    ``close()`` or collection.  ``create`` names the create function where it is not ``eioku_<prefix>_create`` (the flat
    index: ``Handle("index", d, create="eioku_index_flat_create")``), ``device`` goes to ``_lib.init``, and ``lib`` is a
    stand-in for the loaded library (host tests).

    Library functions are called through the handle, which passes itself first: ``h.eioku_yolo_forward(x, n, ...)``.  Once
    closed that raises :class:`EiokuHipError`; NULL never reaches C.  A live handle can also be given to a ctypes call
    as an argument (``_as_parameter_``); ctypes reports a closed one there as its own ``ArgumentError``."""

    def __init__(self, prefix: str, *args, create: str | None = None, device=None, lib=None):
        self._ptr = None
        if lib is None:
            lib = _lib.load()
            _lib.init(device)
        self.lib, self.prefix = lib, prefix
        create = create or f"eioku_{prefix}_create"
        h = C.c_void_p()
        self.check(getattr(lib, create)(*args, C.byref(h)), create)
        self._ptr = h

    # ---- ownership --------------------------------------------------------------------------------------------------
    @property
    def ptr(self) -> C.c_void_p:
        if self._ptr is None:
            raise EiokuHipError(f"the {self.prefix} handle is closed")
        return self._ptr

    _as_parameter_ = ptr

    def __bool__(self) -> bool:
        return self._ptr is not None

    def __getattr__(self, name: str):
        """Only names the instance lacks come here: the library's functions, bound to this handle until ``close()``."""
        if not name.startswith("eioku_"):
            raise AttributeError(name)
        bound = self.__dict__[name] = partial(getattr(self.lib, name), self.ptr)
        return bound

    def close(self) -> None:
        p, self._ptr = self._ptr, None
        for name in [n for n in self.__dict__ if n.startswith("eioku_")]:
            del self.__dict__[name]
        if p is not None:
            getattr(self.lib, f"eioku_{self.prefix}_destroy")(p)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def or_close(self, load, *args, **kw):
        """The rule for "created, but loading failed": ``load(*args, **kw)`` runs, and an exception closes this handle before
        it leaves.  Every owner's constructor runs its loading through here."""
        try:
            return load(*args, **kw)
        except BaseException:
            self.close()
            raise

    def check(self, rc: int, what: str) -> None:
        if rc != 0:
            raise EiokuHipError(f"{what} failed (code {rc}): {(self.lib.eioku_last_error() or b'').decode('utf-8', 'replace')}")

    # ---- the shared families ----------------------------------------------------------------------------------------
    def _table(self, kind: str, ints: int) -> list:
        """``eioku_<prefix>_<kind>_info`` for every index: ``[(name, int, ...)]``, ``None`` for the trailing outputs this
        prefix's function does not have (CRAFT and CRNN report no stride)."""
        what = f"eioku_{self.prefix}_{kind}_info"
        info, name, rows = getattr(self, what), C.create_string_buffer(_NAME), []
        have = len(getattr(self.lib, what).argtypes) - 4
        for i in range(getattr(self, f"eioku_{self.prefix}_num_{kind}s")()):
            out = [C.c_int() for _ in range(have)]
            self.check(info(i, name, _NAME, *map(C.byref, out)), what)
            rows.append((name.value.decode(), *(v.value for v in out), *[None] * (ints - have)))
        return rows

    def convs(self) -> list:
        """``[(name, cout, cin, k, stride)]``."""
        return self._table("conv", 4)

    def tensors(self) -> list:
        """``[(name, rows, cols)]``."""
        return self._table("tensor", 2)

    def set_convs(self, weights) -> None:
        """Weights for every convolution: ``weights`` maps the layer's name to ``(weight, bias)``, or is a callable
        ``(name, cout, cin, k) -> (weight, bias)``.  Shapes must be ``(cout, cin, k, k)`` (or ``(cout, cin)`` when k is 1)
        and ``(cout,)``."""
        set_conv = getattr(self, f"eioku_{self.prefix}_set_conv")
        for i, (name, cout, cin, k, _) in enumerate(self.convs()):
            if callable(weights):
                w, b = weights(name, cout, cin, k)
            elif name in weights:
                w, b = weights[name]
            else:
                raise KeyError(f"state has no weights for {name}")
            w, b = np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
            if (w.shape != (cout, cin, k, k) and (k != 1 or w.shape != (cout, cin))) or b.shape != (cout,):
                raise ValueError(f"{name}: expected weight {(cout, cin, k, k)} and bias {(cout,)}, got {w.shape} and {b.shape}")
            self.check(set_conv(i, w.ctypes.data, b.ctypes.data), f"eioku_{self.prefix}_set_conv({name})")

    def set_tensors(self, weights) -> None:
        """A value for every named tensor: ``weights`` maps the name to an array, or is a callable ``(name, rows, cols) ->
        array``.  Each must have ``rows * cols`` elements."""
        set_tensor = getattr(self, f"eioku_{self.prefix}_set_tensor")
        for i, (name, rows, cols) in enumerate(self.tensors()):
            if callable(weights):
                a = weights(name, rows, cols)
            elif name in weights:
                a = weights[name]
            else:
                raise KeyError(f"state has no weights for {name}")
            a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
            if a.size != rows * cols:
                raise ValueError(f"{name}: expected {rows} x {cols} elements, got {a.size}")
            self.check(set_tensor(i, a.ctypes.data, a.size), f"eioku_{self.prefix}_set_tensor({name})")

    def doubles(self, what: str, n: int = 1) -> tuple:
        """``eioku_<prefix>_<what>(h, &a, &b, ...)`` with ``n`` double outputs (``last_flops``, ``last_ms``) -> floats."""
        out = [C.c_double(0) for _ in range(n)]
        self.check(getattr(self, f"eioku_{self.prefix}_{what}")(*map(C.byref, out)), f"eioku_{self.prefix}_{what}")
        return tuple(v.value for v in out)
