"""Guarded allocations for kernel isolation tests (a plain helper module: no fixture, no pytest setting).

The product carves filters, gradients, momenta, activations and workspaces out of a few flat buffers, back to back,
while a parity test gives every operand its own allocation -- where an overrun of a few hundred bytes lands in
allocator slack.  An `Arena` is ONE allocation, filled with a sentinel word, out of which a test takes every operand,
output and workspace of a launch.  After the launch `check()` asserts that

  * every byte that belongs to no view (the guard bands: >= GUARD bytes before the first view, between two views and
    after the last) still holds the sentinel;
  * every view that was taken with `data` and is not named in `modified` is bit-identical to its host copy
    (operands are frozen);
  * no output (a view taken without `data`, of 4-byte or 8-byte elements, or of 2-byte elements, a byte length that
    is a multiple of 4 and a 4-byte-aligned start) still holds a sentinel word, except where the caller says the
    reference has a NaN.  An 8-byte element (float64, int64) counts as unwritten when BOTH of its 32-bit halves hold
    the sentinel word; 1-byte outputs are not searched (their tests assert the value set themselves).

`untouched(name)` is the query for outputs whose contract is "rows past the count are not written": `nan_ok` excuses
those rows in `check()`, and the test then asserts, word for word, that they still hold the sentinel.

An overrun longer than a guard lands in a neighbouring view; that is still caught, by the frozen-operand check or by
the test's comparison with its oracle.

The sentinel 0x7FC0A5A5 is a quiet NaN with a recognisable payload.  It is written and compared as a bit pattern
(int32 / uint8 views) only: a float fill or a float comparison may canonicalise the payload, and NaN != NaN.

fp16 outputs.  In memory the sentinel word is the two halves 0xA5A5, 0x7FC0: -0.02205 and a NaN.  A fully written,
finite fp16 output cannot contain that pair, so a 2-byte output is searched through its int32 view as well (every
blocked tensor is a multiple of 16 bytes); a `nan_ok` mask given per fp16 element is reduced to one flag per word, and
a word is excused only if the reference has a NaN in either of its halves.  Unwritten padding inside an fp16 pack
therefore holds a NaN in every odd half: a kernel that multiplies padding into a result still fails its comparison.
"""
import numpy as np
import torch

SENTINEL = 0x7FC0A5A5
GUARD = 4096           # bytes of sentinel on each side of every view, at least
ALIGN = 256            # every view starts at a multiple of this (+ its `skew`)

_SENTINEL_BYTES = np.array([SENTINEL], np.uint32).view(np.uint8)        # in memory order


def _up(n, a):
    return (n + a - 1) // a * a


class _View:
    def __init__(self, name, off, nbytes, tensor, host, kind):
        self.name, self.off, self.nbytes, self.tensor, self.host, self.kind = name, off, nbytes, tensor, host, kind


class Arena:
    def __init__(self, nbytes, device="cuda"):
        self.nbytes = _up(int(nbytes), ALIGN)
        raw = torch.empty(self.nbytes + ALIGN, dtype=torch.uint8, device=device)
        base = (-raw.data_ptr()) % ALIGN                 # offsets below are relative to an ALIGN-aligned address
        self.bytes = raw[base:base + self.nbytes]
        self._raw = raw
        self.words = self.bytes.view(torch.int32)
        self.words.fill_(SENTINEL)
        self.device = self.bytes.device
        self.views = []
        self._end = 0                                    # end of the last view
        self._pattern = None

    @staticmethod
    def bytes_for(*sizes):
        """an arena size that holds views of the given byte sizes"""
        return GUARD + sum(_up(int(s), ALIGN) + GUARD + 2 * ALIGN for s in sizes)

    # ---- taking views ------------------------------------------------------------------------------------------

    def _place(self, name, nbytes, skew):
        assert skew >= 0 and skew < ALIGN
        assert all(v.name != name for v in self.views), "view name %r taken twice" % name
        off = _up(self._end + GUARD, ALIGN) + skew
        if off + nbytes + GUARD > self.nbytes:
            raise MemoryError("arena of %d bytes is full: %r needs %d more at offset %d (+ %d of guard)"
                              % (self.nbytes, name, nbytes, off, GUARD))
        self._end = off + nbytes
        return off

    def take(self, shape, dtype, name, data=None, skew=0):
        """A contiguous view of `shape` / `dtype` that starts `skew` bytes after an ALIGN-aligned offset, with at least
        GUARD bytes of sentinel on each side.  data: a numpy array copied in (its host copy is kept as the operand's
        frozen image); without it the view is an output and starts full of sentinel."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        item = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape, dtype=np.int64)) * item
        assert skew % item == 0, "skew must keep the element alignment"
        off = self._place(name, n, skew)
        t = self.bytes[off:off + n].view(dtype).view(shape)
        host = None
        if data is not None:
            host = np.ascontiguousarray(data).copy()
            src = torch.from_numpy(host)
            assert src.dtype == dtype and tuple(src.shape) == shape, (name, src.dtype, dtype, tuple(src.shape), shape)
            t.copy_(src)
        self.views.append(_View(name, off, n, t, host, "input" if data is not None else "output"))
        return t

    def take_bytes(self, n, name):
        """A uint8 workspace view of exactly n bytes (never checked for sentinel left inside: a workspace need not be
        written completely)."""
        n = int(n)
        off = self._place(name, n, 0)
        t = self.bytes[off:off + n]
        self.views.append(_View(name, off, n, t, None, "workspace"))
        return t

    def __getitem__(self, name):
        for v in self.views:
            if v.name == name:
                return v.tensor
        raise KeyError(name)

    # ---- checking ----------------------------------------------------------------------------------------------

    def untouched(self, name):
        """Boolean numpy mask, one flag per 4-byte word of the view `name`, true where the word still holds the
        sentinel: the view's shape for 4-byte elements, shape + (2,) for 8-byte elements, flat otherwise (the byte
        length must then be a multiple of 4).  Synchronises first."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        v = next((v for v in self.views if v.name == name), None)
        assert v is not None, "untouched(): no view named %r" % name
        assert v.nbytes % 4 == 0 and v.off % 4 == 0, "untouched(): view %r is not made of whole words" % name
        left = (self.bytes[v.off:v.off + v.nbytes].view(torch.int32) == SENTINEL).cpu().numpy()
        item = v.tensor.element_size()
        if item == 4:
            return left.reshape(tuple(v.tensor.shape))
        if item == 8:
            return left.reshape(tuple(v.tensor.shape) + (2,))
        return left

    def _nearest(self, a):
        """(view, offset relative to it as text) of absolute arena offset a"""
        best, dist = None, None
        for v in self.views:
            d = v.off - a if a < v.off else a - (v.off + v.nbytes - 1) if a >= v.off + v.nbytes else 0
            if dist is None or d < dist:
                best, dist = v, d
        if best is None:
            return "no view", "arena offset %d" % a
        if a < best.off:
            return best.name, "%d bytes before its start" % (best.off - a)
        return best.name, "%d bytes past its end" % (a - (best.off + best.nbytes))

    def check(self, modified=(), nan_ok=None):
        """Synchronise, then assert the three properties of the module docstring.  modified: names of views taken with
        data that the launch is meant to write.  nan_ok: {output name: boolean numpy mask of the elements where the
        test's reference has a NaN (True = may still hold the sentinel), or True for the whole view}.  Returns True."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        known = {v.name for v in self.views}
        for name in tuple(modified) + tuple(nan_ok or ()):
            assert name in known, "check(): no view named %r" % name
        if self._pattern is None:
            self._pattern = torch.from_numpy(np.tile(_SENTINEL_BYTES, self.nbytes // 4)).to(self.device)
        dirty = self.bytes != self._pattern
        for v in self.views:
            dirty[v.off:v.off + v.nbytes] = False
        if bool(dirty.any()):
            at = torch.nonzero(dirty).flatten().cpu().numpy()
            words = np.unique(at // 4)
            name, rel = self._nearest(int(at[0]))
            last_name, last_rel = self._nearest(int(at[-1]))
            raise AssertionError("guard band overwritten: %d dirty word(s) (%d bytes); the first %s of view %r, the last "
                                 "%s of view %r" % (len(words), len(at), rel, name, last_rel, last_name))
        for v in self.views:
            if v.kind == "input" and v.name not in modified:
                got = v.tensor.detach().cpu().contiguous().numpy().reshape(-1).view(np.uint8)
                want = v.host.reshape(-1).view(np.uint8)
                diff = np.nonzero(got != want)[0]
                if diff.size:
                    raise AssertionError("frozen operand %r modified: %d dirty word(s), the first at byte %d of the view"
                                         % (v.name, len(np.unique(diff // 4)), int(diff[0])))
        for v in self.views:
            item = v.tensor.element_size()
            if v.kind != "output" or not (item in (4, 8) or (item == 2 and v.nbytes % 4 == 0 and v.off % 4 == 0)):
                continue
            ok = (nan_ok or {}).get(v.name)
            if ok is True:
                continue
            if item == 4:
                left = (v.tensor.view(torch.int32) == SENTINEL).cpu().numpy()
                if ok is not None:
                    left &= ~np.asarray(ok, bool).reshape(left.shape)
            elif item == 8:                        # unwritten only if both halves hold the sentinel word
                left = (v.tensor.reshape(-1).view(torch.int32) == SENTINEL).cpu().numpy()
                left = left.reshape(tuple(v.tensor.shape) + (2,)).all(axis=-1)
                if ok is not None:
                    left &= ~np.asarray(ok, bool).reshape(left.shape)
            else:                                  # words of two halves, in memory order
                left = (v.tensor.reshape(-1).view(torch.int32) == SENTINEL).cpu().numpy()
                if ok is not None:
                    left &= ~np.asarray(ok, bool).reshape(-1, 2).any(axis=1)
            if left.any():
                first = int(np.flatnonzero(left)[0])
                raise AssertionError("output %r not written completely: %d word(s) still hold the sentinel, the first at "
                                     "byte %d of the view (element %s)"
                                     % (v.name, int(left.sum()), (8 if item == 8 else 4) * first,
                                        tuple(int(i) for i in np.unravel_index(first, left.shape))))
        return True
