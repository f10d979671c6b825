"""The calling idioms of the C ABI (include/aindex_hip.h), one place each: pointers of arrays and tensors, ragged sequences as bytes and
offsets, the checked call that names its symbol once, the call on torch's current stream, grow-and-retry and size-then-fill outputs,
and malloc'd output blocks taken as numpy arrays. engine.py and engine_graph.py are written in these; nothing here knows an index."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import check, lib, vp


def _np_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(vp)


def _ragged(items: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in items]
    offs = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    return np.frombuffer(b"".join(bs), dtype=np.uint8), offs


def _stream_ptr(device=None):
    """torch's current stream ON `device` (the index's device): the library switches to the handle's device for the call,
    so a stream of whichever device happens to be current would be a stream of the wrong device."""
    import torch
    return vp(torch.cuda.current_stream(device).cuda_stream)


def tptr(t):
    """The address of a tensor's first element, empty or not; None for None (an optional argument left out)."""
    return None if t is None else vp(t.data_ptr())


def tptr_filled(t):
    """tptr, but None for an empty tensor too: for the arguments the library wants null when there is nothing behind them. An empty
    output cut from a buffer that exists — torch.empty(max(n, 1))[:n] — goes through tptr, which passes what torch reports."""
    return None if t is None or not t.numel() else vp(t.data_ptr())


def call(name: str, *args, of=None):
    """lib().<name>(*args), checked; a failure is reported under the symbol, as name(of) when the caller says what it was working on."""
    check(getattr(lib(), name)(*args), name if of is None else f"{name}({of})")


def dev_call(device, name: str, *args):
    """call() of a `_dev` entry point: on `device` (the index's), its last argument torch's current stream there."""
    import torch
    with torch.cuda.device(device):
        call(name, *args, _stream_ptr(device))


def grow_retry(name: str, dtypes, device, cap_hint: int, fn):
    """Outputs whose length only the call itself knows: fn(pointers, cap, byref(total)) -> status fills one tensor per dtype of cap
    entries each and reports the entries there are. The first attempt makes room for cap_hint entries (null pointers when that is 0: a
    sizing pass), a second one, when the total is larger, for exactly the total. -> (the tensors cut to total, total)."""
    import torch
    total = C.c_uint64()
    cap = max(int(cap_hint), 0)
    while True:
        outs = [torch.empty(max(cap, 1), dtype=dt, device=device) for dt in dtypes]
        check(fn([vp(o.data_ptr()) if cap else None for o in outs], cap, C.byref(total)), name)
        if total.value <= cap:
            break
        cap = total.value
    return [o[:total.value] for o in outs], total.value


def dev_grow_retry(device, name: str, dtypes, cap_hint: int, args):
    """grow_retry of a `_dev` entry point on `device`: args(pointers, cap, byref(total)) -> its arguments but the stream."""
    import torch
    f, st = getattr(lib(), name), _stream_ptr(device)
    with torch.cuda.device(device):
        return grow_retry(name, dtypes, f"cuda:{device}", cap_hint, lambda o, cap, tot: f(*args(o, cap, tot), st))


def dev_size_then_fill(device, name: str, n_offsets: int, dtypes, args):
    """CSR outputs of a `_dev` entry point on `device`: the sizing call (null outputs, room for 0) fills offsets int64[n_offsets] and
    reports the total, the filling call — left out when the total is 0 — writes one tensor per dtype of exactly that size.
    args(offsets pointer, pointers, cap, byref(total)) -> its arguments but the stream. -> (offsets, the tensors)."""
    import torch
    dev = f"cuda:{device}"
    offsets = torch.empty(n_offsets, dtype=torch.int64, device=dev)
    total = C.c_uint64()
    f, st = getattr(lib(), name), _stream_ptr(device)
    with torch.cuda.device(device):
        check(f(*args(tptr(offsets), [None] * len(dtypes), 0, C.byref(total)), st), name)
        t = total.value
        outs = [torch.empty(max(t, 1), dtype=dt, device=dev)[:t] for dt in dtypes]
        if t:
            check(f(*args(tptr(offsets), [tptr(o) for o in outs], t, C.byref(total)), st), name)
    return offsets, outs


def take(p, n: int, dtype=np.uint64) -> np.ndarray:
    """n entries of a malloc'd output block of the C ABI as a numpy array of its own; the block is freed."""
    dt = np.dtype(dtype)
    try:
        return np.frombuffer(C.string_at(p, dt.itemsize * n), dtype=dt).copy() if n else np.zeros(0, dt)
    finally:
        lib().aix_free(p)


def take_table(ps, names, sizes, dtypes) -> dict:
    """{name: take(block, size, dtype)} over the output blocks of a host form, in order; a size of None is an output that was not
    asked for (no block, None). Every block is freed, also when one of them cannot be taken."""
    out, left = {}, [p for p, n in zip(ps, sizes) if n is not None]
    try:
        for name, n, dt in zip(names, sizes, dtypes):
            out[name] = take(left.pop(0), n, dt) if n is not None else None
    finally:
        for p in left:
            lib().aix_free(p)
    return out
