"""Volumes far out in one large buffer (tests/test_gpu_far_pool.py, tests/test_far_pool_cpu.py): the constants of the placements,
`relocate` for every kind of offset table, and the helpers that fill and check the buffer.  Importing this needs numpy only.

Every volume of this project lies at a 64-bit ELEMENT offset in a flat buffer (omgx_object.grid_offset, omgx_mesh.out_offset,
state_begin / comp_begin / out_begin) and a node inside a volume has a 32-bit index.  The tests run a call on a compact table and
on the same table moved to a far base, and ask for the same bits.

WHY EXACTLY THESE PLACEMENTS.  A test here must not be able to fault the device even when the kernel under test is wrong: a wrong
kernel has to read or write the wrong place INSIDE the allocation.  The buffer has 2^32 + RESERVE float32 elements and the bases are
    B1 = 2^30 + K   (the BYTE offset of a float32 element no longer fits in 32 bits)
    B2 = 2^32 + K   (the ELEMENT offset no longer fits in 32 bits)
with K = 4099: small, odd (8- and 16-byte loads are exercised unaligned to their size) and not smaller than the guard band.  With
these bases an element or byte offset cut to 32 bits, read as signed or as unsigned, is K + i elements: inside the ALIAS WINDOW
[0, K + used + BAND) of the same buffer.  So
  * there is no placement near 2^31 elements,
  * no placement straddles 2^30 or 2^32 elements,
  * no base pointer lies outside a real allocation:
under a sign-wrapped index each of those would leave the allocation and turn a failing test into a GPU fault.  Do not add one.

READERS find the real content at the far base and DIFFERENT, finite, plausible content in the alias window (`alias_content`: the
volumes negated, states with free and surface swapped), so a wrapped read gives other bits, not NaNs.  WRITERS find a guard pattern
in the alias window and in a band of BAND elements before and after every far volume; afterwards both must hold exactly the pattern.

Several arrays of one call (a state array, a pool, tsdf and weight) share the buffer as LANES: views of VIEW elements that start
16 MiB apart, so that neither their far regions nor their alias windows overlap (`lane`; one lane number per array and call)."""
from __future__ import annotations

import ctypes as C

import numpy as np

K = 4099                      # the small odd offset of both bases, >= BAND
BAND = 4096                   # guard elements before and after each far volume
B1 = (1 << 30) + K            # byte offsets of float32 elements pass 2^32
B2 = (1 << 32) + K            # element offsets pass 2^32
BASES = (B1, B2)
RESERVE = 32 << 20            # R: elements behind 2^32
ELEMS = (1 << 32) + RESERVE   # float32 elements of the buffer: 16.1 GiB
LANE = 4 << 20                # 4-byte elements between the starts of two lanes (16 MiB)
LANES = 4
VIEW = (1 << 32) + (16 << 20)  # elements of a lane, of whatever type
MAX_USED = LANE - K - BAND    # elements one array of a call may use, so that no alias window reaches the next lane
HEADROOM = 2 << 30            # bytes that must stay free beside the buffer

GUARD32 = 0x5A5A5A5A          # as float32 1.5e16, as int32 a label no volume has
GUARD8 = 0x5A                 # a state byte that is none of 0, 1, 2

assert K >= BAND and K % 2 == 1 and RESERVE <= 32 << 20 and (LANES - 1) * LANE + VIEW <= ELEMS and B2 + MAX_USED + BAND <= VIEW


def relocate(records, delta: int):
    """A copy of an offset table moved by `delta` elements, in 64 bits; nothing but the offsets changes.
      * a numpy record array with a `grid_offset` field (scenes.OBJECT_DTYPE): grid_offset + delta;
      * a ctypes array of omgx_mesh records (ops.surface_records, RayBatch.rec): out_offset + delta;
      * a list of volume layouts (origin, delta, sample, dims, offset): the fifth field + delta;
      * an integer array (state_begin, comp_begin, out_begin, out_offsets): every element + delta, as int64."""
    delta = int(delta)
    if isinstance(records, np.ndarray) and records.dtype.names and "grid_offset" in records.dtype.names:
        assert records.dtype["grid_offset"] == np.int64
        out = records.copy()
        out["grid_offset"] = records["grid_offset"].astype(np.int64) + np.int64(delta)
        return out
    if isinstance(records, C.Array) and hasattr(records._type_, "out_offset"):
        out = type(records)()
        C.memmove(out, records, C.sizeof(records))
        for r in out:
            r.out_offset = int(r.out_offset) + delta
        return out
    if isinstance(records, (list, tuple)) and len(records) and isinstance(records[0], (list, tuple)):
        assert all(len(v) == 5 for v in records), "a layout needs its offset to be moved"
        return [tuple(v[:4]) + (int(v[4]) + delta,) for v in records]
    a = np.asarray(records)
    assert a.dtype.kind in "iu", a.dtype
    return a.astype(np.int64) + np.int64(delta)


def spread(sizes, gap: int = BAND):
    """(offsets, used): volumes of `sizes` elements from offset 0 with `gap` elements between them, so that every far volume has
    its own guard band (the bands before the first and behind the last are the far region's own)."""
    offsets, at = [], 0
    for n in sizes:
        offsets.append(at)
        at += int(n) + gap
    return offsets, at - gap if sizes else 0


def alias_content(compact: np.ndarray) -> np.ndarray:
    """What the alias window holds for readers: different, finite and plausible.  float: the volumes negated (inside and outside
    change places); uint8 states: free (0) and surface (1) swapped; other integers: the order reversed."""
    a = np.ascontiguousarray(compact)
    if a.dtype.kind == "f":
        out = -a
        out[a == 0] = 1.0  # (-0.0 reads as 0.0 through every kernel)
        return out
    if a.dtype == np.uint8:
        return np.where(a == 0, 1, np.where(a == 1, 0, a)).astype(np.uint8)
    return np.ascontiguousarray(a[::-1])


_FILLER = {"f": 1.0, "u": 2, "i": -1}  # what lies around the real and the alias content of a reader: finite, unknown, no label


def _torch():
    import torch
    return torch


def lane(buffer, j: int, dtype=None):
    """Lane j of the buffer as a flat view of VIEW elements of `dtype` (float32, int32 or uint8) that starts j * 16 MiB into it."""
    torch = _torch()
    dtype = torch.float32 if dtype is None else dtype
    assert 0 <= j < LANES and buffer.dtype == torch.float32 and buffer.dim() == 1 and buffer.numel() >= (LANES - 1) * LANE + VIEW
    if dtype == torch.uint8:
        return buffer.view(torch.uint8)[4 * j * LANE: 4 * j * LANE + VIEW]
    assert dtype in (torch.float32, torch.int32)
    flat = buffer if dtype == torch.float32 else buffer.view(torch.int32)
    return flat[j * LANE: j * LANE + VIEW]


def _check_span(view, base: int, used: int):
    # (a small buffer, as the CPU tests use, cannot be left by a 32-bit wrap of an index that fits it: any base goes there)
    assert base in BASES or view.numel() <= 1 << 24, "see the module's docstring before adding a placement"
    assert 0 <= used <= MAX_USED and base >= K >= BAND and base + used + BAND <= view.numel()


def place(view, compact, base: int):
    """Readers.  Copy the compact content (a numpy array of the view's type) to view[base : base + n], put alias_content() at
    view[K : K + n], and a finite filler over the rest of the alias window and over a band before and after the far content.
    -> n."""
    torch = _torch()
    a = np.ascontiguousarray(compact).reshape(-1)
    n = a.size
    _check_span(view, base, n)
    assert torch.from_numpy(a[:0]).dtype == view.dtype, (a.dtype, view.dtype)
    fill = _FILLER[a.dtype.kind]
    view[: K + n + BAND].fill_(fill)
    view[K: K + n].copy_(torch.from_numpy(alias_content(a)))
    view[base - BAND: base + n + BAND].fill_(fill)
    view[base: base + n].copy_(torch.from_numpy(a))
    return n


def _bits(view):
    torch = _torch()
    return view if view.dtype in (torch.uint8, torch.int32) else view.view(torch.int32)


def guard_value(view):
    return GUARD8 if view.dtype == _torch().uint8 else GUARD32


def guard(view, base: int, used: int):
    """Writers.  The guard pattern over the alias window [0, K + used + BAND) and over [base - BAND, base + used + BAND)."""
    _check_span(view, base, used)
    b = _bits(view)
    b[: K + used + BAND].fill_(guard_value(view))
    b[base - BAND: base + used + BAND].fill_(guard_value(view))


def guard_compact(n: int, like, device):
    """A compact buffer of n elements of `like`'s type that holds the guard pattern: what a writer's compact run writes into."""
    torch = _torch()
    out = torch.empty(n, dtype=like.dtype, device=device)
    _bits(out).fill_(guard_value(out))
    return out


def written(view, base: int, compact) -> dict:
    """After a writer ran on the far table: {"far": the far region holds the compact run's bits (the gaps between the volumes
    included: they hold the guard in both), "bands": the bands before and behind it hold the guard, "alias": so does the alias
    window}.  compact: the compact run's buffer, which started as guard_compact()."""
    torch = _torch()
    c, b, g = _bits(compact.reshape(-1)), _bits(view), guard_value(view)
    n = c.numel()
    return {"far": bool(torch.equal(b[base: base + n], c)),
            "bands": bool((b[base - BAND: base] == g).all()) and bool((b[base + n: base + n + BAND] == g).all()),
            "alias": bool((b[: K + n + BAND] == g).all())}
