"""Device-resident stripes: plans over shards already in HBM.

A *stripe* is one object's n = k+m shards. `StripeBatch` lays a batch of stripes out
in HBM: by default in one allocation, `[batch][n][pitch]` bytes (pitch = S rounded up to
256 B so every shard starts 16-B aligned for the vector kernel), the layout the GPU
tests use; the benchmark's `planar` layout keeps the data shards and the parity in two
regions, and the Split layouts reproduce upstream's (see the class). `Plan` wraps rs_plan_create/rs_plan_launch: the
coefficient tables and shard-pointer tables are uploaded once, and each launch only
enqueues kernels on the given stream (capturable in a HIP graph).

PyTorch is only the allocator and stream provider here; the arithmetic is the HIP
kernels in libcallfs_rs.so.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _native as N


def pitch_for(S: int) -> int:
    return (S + 255) // 256 * 256


def _aligned_empty(shape, align: int, device) -> torch.Tensor:
    """An uninitialised uint8 tensor of `shape` whose first byte is `align`-aligned."""
    n = 1
    for d in shape:
        n *= d
    raw = torch.empty(n + align, dtype=torch.uint8, device=device)
    off = -raw.data_ptr() % align
    return raw[off:off + n].view(shape)


class StripeBatch:
    """`batch` stripes of RS(k, m) with shard size S, resident on `device`.

    layout "pitch" (default): shards at a 256-B pitch, every shard 16-B aligned.
    layout "split": upstream `Split`'s layout of contiguous objects (codec.go:31) when the
    body's capacity holds all n shards: pitch = S, object b's shard i at b*n*S + i*S, so
    at odd S every shard but the first sits at its own byte offset (the realigning
    kernel's case).
    layout "planar": the pitch layout's 256-B shard pitch, but the k data shards of every
    stripe in one region ([batch][k][pitch]) and the m parity shards in another
    ([batch][m][pitch]), so no stripe's parity sits between two stripes' data.
    layout "shardmajor": the 256-B pitch with all stripes' shard i in one region
    ([n][batch][pitch]).
    layout "readall": upstream `Split` of a body whose capacity holds the k data shards
    but not the parity, which is what CallFS passes it: io.ReadAll's body
    (post_file_enhanced.go:127) grows by append, so cap/len stays below n/k for every
    profile with m/k > 1/4. The data shards are slices of the body at pitch S (body
    bases `BODY_ALIGN`-aligned, as the Go heap's large objects are page-aligned); the m
    parity shards come from reedsolomon's AllocAligned: 64-B aligned, each at a pitch of
    S rounded up to 64 B (klauspost/reedsolomon v1.13.3 reedsolomon.go Split,
    galois.go AllocAligned)."""

    BODY_ALIGN = 8192

    def __init__(self, k: int, m: int, S: int, batch: int, device: torch.device,
                 layout: str = "pitch", pitch: Optional[int] = None):
        """pitch: shard pitch in bytes for the 'pitch', 'planar' and 'shardmajor' layouts
        (a multiple of 16, at least S; default pitch_for(S), the library's own rule)."""
        if layout not in ("pitch", "split", "readall", "planar", "shardmajor"):
            raise ValueError(f"layout {layout!r}")
        if pitch is not None and (layout in ("split", "readall") or pitch < S or pitch % 16):
            raise ValueError(f"pitch {pitch} for layout {layout!r}, S = {S}")
        self.k, self.m, self.S, self.batch = k, m, S, batch
        self.n = k + m
        self.layout = layout
        self.device = torch.device(device)
        if layout in ("readall", "planar"):
            # data shard i of stripe b at body + b*body_pitch + i*pitch, parity j at
            # par + (b*m + j)*par_pitch
            if layout == "readall":
                self.pitch = S
                self.body_pitch = -(-k * S // self.BODY_ALIGN) * self.BODY_ALIGN
                self.par_pitch = -(-S // 64) * 64
            else:
                self.pitch = self.par_pitch = pitch or pitch_for(S)
                self.body_pitch = k * self.pitch
            self.body = _aligned_empty((batch, self.body_pitch), self.BODY_ALIGN, self.device)
            self.par = _aligned_empty((batch, m, self.par_pitch), 256, self.device)
            self.buf = None
            return
        self.pitch = S if layout == "split" else (pitch or pitch_for(S))
        if layout == "shardmajor":
            sm = torch.empty((self.n, batch, self.pitch), dtype=torch.uint8, device=self.device)
            self.buf = sm.permute(1, 0, 2)  # [batch][n][pitch] view of [n][batch][pitch]
            return
        self.buf = torch.empty((batch, self.n, self.pitch), dtype=torch.uint8, device=self.device)

    def shard(self, b: int, i: int) -> torch.Tensor:
        if self.buf is None:
            if i < self.k:
                return self.body[b, i * self.pitch:i * self.pitch + self.S]
            return self.par[b, i - self.k, : self.S]
        return self.buf[b, i, : self.S]

    def data(self) -> torch.Tensor:
        if self.buf is None:
            return self.body[:, : self.k * self.pitch].view(self.batch, self.k, self.pitch)[:, :, : self.S]
        return self.buf[:, : self.k, : self.S]

    def parity(self) -> torch.Tensor:
        if self.buf is None:
            return self.par[:, :, : self.S]
        return self.buf[:, self.k:, : self.S]

    def gather(self, stripes: Optional[int] = None) -> torch.Tensor:
        """A [stripes][n][S] copy of the first `stripes` stripes' shards (all by default)."""
        ns = self.batch if stripes is None else stripes
        if self.buf is None:
            return torch.cat([self.data()[:ns], self.parity()[:ns]], dim=1)
        return self.buf[:ns, :, : self.S].clone()

    def zero_shard(self, i: int) -> None:
        """Zero shard i of every stripe."""
        if self.buf is None:
            (self.data()[:, i] if i < self.k else self.parity()[:, i - self.k]).zero_()
        else:
            self.buf[:, i, : self.S].zero_()

    def pointers(self) -> list:
        if self.buf is None:
            body, par = self.body.data_ptr(), self.par.data_ptr()
            return [body + b * self.body_pitch + i * self.pitch if i < self.k
                    else par + (b * self.m + i - self.k) * self.par_pitch
                    for b in range(self.batch) for i in range(self.n)]
        base = self.buf.data_ptr()
        sb_, si_ = self.buf.stride(0), self.buf.stride(1)
        return [base + b * sb_ + i * si_ for b in range(self.batch) for i in range(self.n)]

    def fill_random(self, seed: int) -> None:
        g = torch.Generator(device=self.device)
        g.manual_seed(seed)
        for t in ((self.buf,) if self.buf is not None else (self.body, self.par)):
            t.random_(0, 256, generator=g)


class RaggedBatch:
    """Stripes of RS(k, m) with their own shard sizes (`sizes[b]` bytes for every shard of
    stripe b), resident on `device` in one allocation, stripe after stripe and shard after
    shard (the input of a ragged plan).

    layout "aligned" (default): each shard starts at the next 256-B boundary.
    layout "packed": shards back to back with no padding, so odd sizes give misaligned
    addresses and adjacent shards touch."""

    def __init__(self, k: int, m: int, sizes: Sequence[int], device: torch.device,
                 layout: str = "aligned"):
        if layout not in ("aligned", "packed"):
            raise ValueError(f"layout {layout!r}")
        self.k, self.m, self.n = k, m, k + m
        self.sizes = [int(s) for s in sizes]
        if not self.sizes or min(self.sizes) < 1:
            raise ValueError("sizes: at least one stripe, every shard size >= 1")
        self.batch = len(self.sizes)
        self.layout = layout
        self.device = torch.device(device)
        self.offsets = []  # [batch][n] byte offset of each shard in buf
        off = 0
        for S in self.sizes:
            row = []
            for _ in range(self.n):
                if layout == "aligned":
                    off = (off + 255) // 256 * 256
                row.append(off)
                off += S
            self.offsets.append(row)
        self.nbytes = off
        self.buf = _aligned_empty((off,), 256, self.device)

    def shard(self, b: int, i: int) -> torch.Tensor:
        o = self.offsets[b][i]
        return self.buf[o:o + self.sizes[b]]

    def pointers(self) -> list:
        base = self.buf.data_ptr()
        return [base + o for row in self.offsets for o in row]

    def fill_random(self, seed: int) -> None:
        g = torch.Generator(device=self.device)
        g.manual_seed(seed)
        self.buf.random_(0, 256, generator=g)

    def gather_stripe(self, b: int) -> torch.Tensor:
        """An [n][sizes[b]] copy of stripe b's shards."""
        return torch.stack([self.shard(b, i) for i in range(self.n)])


def _mask_rows(present):
    """The rows of a per-stripe presence mask (a batch x n sequence or array), or None
    when `present` is None or a flat sequence of flags."""
    if present is None:
        return None
    if hasattr(present, "ndim"):  # numpy array or torch tensor
        if present.ndim == 1:
            return None
        if present.ndim != 2:
            raise ValueError("present: n flags, or batch rows of n flags")
        return present.tolist()
    rows = list(present)
    if rows and all(hasattr(r, "__len__") for r in rows):
        return [list(r) for r in rows]
    if any(hasattr(r, "__len__") for r in rows):
        raise ValueError("present: n flags, or batch rows of n flags")
    return None


class Plan:
    """rs_plan over explicit device shard pointers (batch*n of them, stripe-major).

    present=None is an encode plan (data present, parity missing); otherwise the
    missing shards are reconstructed from the first k present ones and the remaining
    present parity is re-verified (codec.go:55,59). A flat sequence of k+m flags is one
    mask for the whole batch; a batch x (k+m) sequence or array gives every stripe its own
    mask (a mixed plan, DESIGN.md §5.8: one launch repairs stripes with different erasures).
    `Plan.ragged` builds a plan over stripes of different shard sizes,
    `Plan.locate` one that tells which shard of a stripe is corrupt (§5.12), `Plan.correct` one
    that repairs single corrupt bytes in place (§5.13).
    """

    def __init__(self, k: int, m: int, S: int, batch: int, pointers: Sequence[int],
                 present: Optional[Sequence[bool]] = None, device: int = 0,
                 context: Optional[N.Context] = None):
        self.ctx = context or N.default_context()
        n = k + m
        if len(pointers) != batch * n:
            raise ValueError("need batch*(k+m) shard pointers")
        self.k, self.m, self.S, self.batch, self.device = k, m, S, batch, device
        ptrs = (ctypes.c_void_p * len(pointers))(*pointers)
        pres = None
        h = ctypes.c_void_p()
        rows = _mask_rows(present)
        if rows is not None:
            # batch x n flags: a mixed plan, every stripe its own mask (rs_plan_create_mixed)
            if len(rows) != batch or any(len(r) != n for r in rows):
                raise ValueError("a per-stripe present needs batch rows of k+m flags")
            flat = [1 if p else 0 for r in rows for p in r]
            pres = (ctypes.c_uint8 * (batch * n))(*flat)
            N.check(N.lib.rs_plan_create_mixed(self.ctx.handle, device, k, m, S, batch, pres, ptrs,
                                               ctypes.byref(h)), "rs_plan_create_mixed")
            self.handle = h
            return
        if present is not None:
            if len(present) != n:
                raise ValueError("present needs k+m flags")
            pres = (ctypes.c_uint8 * n)(*[1 if p else 0 for p in present])
        N.check(N.lib.rs_plan_create(self.ctx.handle, device, k, m, S, batch, pres, ptrs,
                                     ctypes.byref(h)), "rs_plan_create")
        self.handle = h

    @classmethod
    def for_batch(cls, sb: StripeBatch, present=None, context=None) -> "Plan":
        dev = sb.device.index if sb.device.index is not None else 0
        return cls(sb.k, sb.m, sb.S, sb.batch, sb.pointers(), present, dev, context)

    @classmethod
    def ragged(cls, k: int, m: int, sizes: Sequence[int], pointers: Sequence[int],
               present=None, device: int = 0, context: Optional[N.Context] = None,
               required=None) -> "Plan":
        """rs_plan_create_ragged: stripe b's shards are sizes[b] bytes; one
        launch encodes, repairs and verifies stripes of different shard sizes. present: None
        (every stripe an encode) or batch rows of k+m flags. The plan's S is None and its
        sizes are kept; when all sizes are equal the library builds the mixed (or uniform)
        plan of that size.
        required: None, or batch rows of k+m flags beside present's
        (rs_plan_create_required): a missing shard whose flag is clear is
        neither rebuilt nor touched (its pointer may be 0)."""
        n, batch = k + m, len(sizes)
        if len(pointers) != batch * n:
            raise ValueError("need batch*(k+m) shard pointers")
        pres = None
        if present is not None:
            rows = _mask_rows(present)
            if rows is None or len(rows) != batch or any(len(r) != n for r in rows):
                raise ValueError("present: None, or batch rows of k+m flags")
            pres = (ctypes.c_uint8 * (batch * n))(*[1 if p else 0 for r in rows for p in r])
        req = None
        if required is not None:
            rows = _mask_rows(required)
            if rows is None or len(rows) != batch or any(len(r) != n for r in rows):
                raise ValueError("required: None, or batch rows of k+m flags")
            req = (ctypes.c_uint8 * (batch * n))(*[1 if p else 0 for r in rows for p in r])
        self = cls.__new__(cls)
        self.ctx = context or N.default_context()
        self.k, self.m, self.S, self.batch, self.device = k, m, None, batch, device
        self.sizes = [int(s) for s in sizes]
        self.handle = None
        ptrs = (ctypes.c_void_p * max(1, len(pointers)))(*pointers)
        szs = (ctypes.c_size_t * max(1, batch))(*self.sizes)
        h = ctypes.c_void_p()
        if req is not None:
            N.check(N.lib.rs_plan_create_required(self.ctx.handle, device, k, m, batch, szs, pres,
                                                  req, ptrs, ctypes.byref(h)),
                    "rs_plan_create_required")
        else:
            N.check(N.lib.rs_plan_create_ragged(self.ctx.handle, device, k, m, batch, szs, pres,
                                                ptrs, ctypes.byref(h)), "rs_plan_create_ragged")
        self.handle = h
        return self

    @classmethod
    def for_ragged(cls, rb: "RaggedBatch", present=None, context=None, required=None,
                   locate: bool = False, max_errors: int = 1) -> "Plan":
        dev = rb.device.index if rb.device.index is not None else 0
        if locate:
            if required is not None:
                raise ValueError("a locate plan writes nothing: no required set")
            return cls.locate(rb.k, rb.m, rb.sizes, rb.pointers(), present, dev, context, max_errors)
        if max_errors != 1:
            raise ValueError("max_errors belongs to a locate plan")
        return cls.ragged(rb.k, rb.m, rb.sizes, rb.pointers(), present, dev, context, required)

    @classmethod
    def locate(cls, k: int, m: int, sizes: Sequence[int], pointers: Sequence[int],
               present=None, device: int = 0, context: Optional[N.Context] = None,
               max_errors: int = 1) -> "Plan":
        """rs_plan_create_locate(_ex): a plan that writes nothing and tells
        which shard of a stripe is corrupt. present: None (every shard present) or batch rows of
        k+m flags. A launch compares each stripe's present shards beyond the first k (16 at the
        most) and classifies every mismatching byte column; `blame()` reads the counts.
        max_errors=2 (§5.12.1): a stripe that compares four or more shards also names the two
        shards of a column in which two are corrupt; such a column counts once for each."""
        return cls._locate_like(k, m, sizes, pointers, present, device, context, max_errors, False)

    @classmethod
    def correct(cls, k: int, m: int, sizes: Sequence[int], pointers: Sequence[int],
                present=None, device: int = 0, context: Optional[N.Context] = None) -> "Plan":
        """rs_plan_create_correct: a locate plan whose launch repairs what it
        blames. In a stripe that compares three or more shards, a byte column in which one
        examined shard is corrupt gets that byte restored IN PLACE (the shard pointers are
        written through, the k read shards included); columns with more errors, and every
        mismatching column of a stripe that compares fewer than three shards, are left as they
        are. `blame()` reads the counts: [b, i] = bytes of shard i of stripe b the launches
        changed, [b, k+m] = columns left mismatching."""
        return cls._locate_like(k, m, sizes, pointers, present, device, context, 1, True)

    @classmethod
    def _locate_like(cls, k, m, sizes, pointers, present, device, context, max_errors, correct) -> "Plan":
        n, batch = k + m, len(sizes)
        if len(pointers) != batch * n:
            raise ValueError("need batch*(k+m) shard pointers")
        pres = None
        if present is not None:
            rows = _mask_rows(present)
            if rows is None or len(rows) != batch or any(len(r) != n for r in rows):
                raise ValueError("present: None, or batch rows of k+m flags")
            pres = (ctypes.c_uint8 * (batch * n))(*[1 if p else 0 for r in rows for p in r])
        self = cls.__new__(cls)
        self.ctx = context or N.default_context()
        self.k, self.m, self.S, self.batch, self.device = k, m, None, batch, device
        self.sizes = [int(s) for s in sizes]
        self.handle = None
        ptrs = (ctypes.c_void_p * max(1, len(pointers)))(*pointers)
        szs = (ctypes.c_size_t * max(1, batch))(*self.sizes)
        h = ctypes.c_void_p()
        if correct:
            N.check(N.lib.rs_plan_create_correct(self.ctx.handle, device, k, m, batch, szs, pres, ptrs,
                                                 ctypes.byref(h)), "rs_plan_create_correct")
        elif max_errors == 1:
            N.check(N.lib.rs_plan_create_locate(self.ctx.handle, device, k, m, batch, szs, pres, ptrs,
                                                ctypes.byref(h)), "rs_plan_create_locate")
        else:
            N.check(N.lib.rs_plan_create_locate_ex(self.ctx.handle, device, k, m, batch, szs, pres, ptrs,
                                                   int(max_errors), ctypes.byref(h)),
                    "rs_plan_create_locate_ex")
        self.handle = h
        return self

    def blame(self, stream: Optional[torch.cuda.Stream] = None):
        """rs_plan_blame of a locate plan (or a correct plan: bytes changed per shard, and the
        columns left mismatching): synchronises the stream and returns a
        (batch, k+m+1) uint64 array: [b, i] = byte columns of stripe b blamed on shard i,
        [b, k+m] = its unexplained columns (a pair plan counts a column blamed on two shards
        once for each). Clears the counts; launches accumulate until the
        next read, so two launches before one read give every count doubled."""
        import numpy as np
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        out = np.zeros((self.batch, self.k + self.m + 1), dtype=np.uint64)
        N.check(N.lib.rs_plan_blame(self.handle, ctypes.c_void_p(s.cuda_stream),
                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))),
                "rs_plan_blame")
        return out

    @classmethod
    def update(cls, k: int, m: int, sizes: Sequence[int], changed, old_ptrs, new_ptrs,
               parity_ptrs, device: int = 0, context: Optional[N.Context] = None) -> "Plan":
        """rs_plan_create_update: upstream Update / EncodeIdx on device
        memory. changed: batch rows of k flags; old_ptrs / new_ptrs: batch*k device pointers
        (read where changed; 0 elsewhere is fine), parity_ptrs: batch*m. old_ptrs=None is
        EncodeIdx mode: the flagged new shards' products are added to the parity. A launch
        sets parity ^= P[:, changed] * (old ^ new) in place. NOT idempotent: a second launch
        applies the delta again and restores the parity the first started from."""
        batch = len(sizes)
        rows = _mask_rows(changed)
        if rows is None or len(rows) != batch or any(len(r) != k for r in rows):
            raise ValueError("changed: batch rows of k flags")
        if len(new_ptrs) != batch * k or len(parity_ptrs) != batch * m or (
                old_ptrs is not None and len(old_ptrs) != batch * k):
            raise ValueError("need batch*k old / new pointers and batch*m parity pointers")
        self = cls.__new__(cls)
        self.ctx = context or N.default_context()
        self.k, self.m, self.S, self.batch, self.device = k, m, None, batch, device
        self.sizes = [int(s) for s in sizes]
        self.handle = None
        flags = (ctypes.c_uint8 * max(1, batch * k))(*[1 if f else 0 for r in rows for f in r])
        szs = (ctypes.c_size_t * max(1, batch))(*self.sizes)
        arr = lambda p: (ctypes.c_void_p * max(1, len(p)))(*p)  # noqa: E731
        h = ctypes.c_void_p()
        N.check(N.lib.rs_plan_create_update(self.ctx.handle, device, k, m, batch, szs, flags,
                                            None if old_ptrs is None else arr(old_ptrs),
                                            arr(new_ptrs), arr(parity_ptrs), ctypes.byref(h)),
                "rs_plan_create_update")
        self.handle = h
        return self

    @classmethod
    def decode_idx(cls, k: int, m: int, sizes: Sequence[int], expect, input_ptrs, dst_ptrs,
                   store: bool = False, device: int = 0,
                   context: Optional[N.Context] = None) -> "Plan":
        """rs_plan_create_decode_idx: upstream DecodeIdx on device memory.
        expect: batch rows of k+m flags, exactly k set per row: the shards the decode will be
        fed over all plans. input_ptrs: batch*(k+m) device pointers, nonzero = delivered with
        this plan (expected indices only); dst_ptrs: batch*(k+m), nonzero = wanted (indices that
        are not expected only). A launch adds C[:, delivered] * inputs into the wanted shards
        (C = E[wanted] * inv(E[expected])), or with store=True stores it without reading them.
        After every expected shard has been delivered once the wanted shards hold what a
        reconstruct from those k shards gives. A merge launch is NOT idempotent."""
        batch = len(sizes)
        n = k + m
        rows = _mask_rows(expect)
        if rows is None or len(rows) != batch or any(len(r) != n for r in rows):
            raise ValueError("expect: batch rows of k+m flags")
        if len(input_ptrs) != batch * n or len(dst_ptrs) != batch * n:
            raise ValueError("need batch*(k+m) input pointers and batch*(k+m) dst pointers")
        self = cls.__new__(cls)
        self.ctx = context or N.default_context()
        self.k, self.m, self.S, self.batch, self.device = k, m, None, batch, device
        self.sizes = [int(s) for s in sizes]
        self.handle = None
        flags = (ctypes.c_uint8 * max(1, batch * n))(*[1 if f else 0 for r in rows for f in r])
        szs = (ctypes.c_size_t * max(1, batch))(*self.sizes)
        arr = lambda p: (ctypes.c_void_p * max(1, len(p)))(*[int(x) or None for x in p])  # noqa: E731
        h = ctypes.c_void_p()
        N.check(N.lib.rs_plan_create_decode_idx(self.ctx.handle, device, k, m, batch, szs, flags,
                                                arr(input_ptrs), arr(dst_ptrs),
                                                N.RS_DECODE_IDX_STORE if store else 0,
                                                ctypes.byref(h)),
                "rs_plan_create_decode_idx")
        self.handle = h
        return self

    @classmethod
    def decode_check(cls, k: int, m: int, sizes: Sequence[int], expect, input_ptrs, dst_ptrs, check_ptrs,
                     store: bool = False, final: bool = False, device: int = 0,
                     context: Optional[N.Context] = None) -> "Plan":
        """rs_plan_create_decode_check: a decode_idx plan that also keeps, per
        compared shard, a syndrome accumulator. check_ptrs: batch*(k+m) device pointers, nonzero =
        shard i is compared and this is its accumulator (indices that are neither expected nor
        wanted only); input_ptrs may then also deliver shard i itself. A launch adds the delivered
        expected shards' terms, and the compared shard when delivered, into the accumulator (or
        stores them with store=True). final=True writes no accumulator: the value it would have
        received is tested and a nonzero byte flags the stripe (corrupt(), corrupt_stripes());
        with store=True as well the accumulators are not read either. A non-final merge launch is
        NOT idempotent."""
        batch = len(sizes)
        n = k + m
        rows = _mask_rows(expect)
        if rows is None or len(rows) != batch or any(len(r) != n for r in rows):
            raise ValueError("expect: batch rows of k+m flags")
        if len(input_ptrs) != batch * n or len(dst_ptrs) != batch * n or len(check_ptrs) != batch * n:
            raise ValueError("need batch*(k+m) input, dst and check pointers each")
        self = cls.__new__(cls)
        self.ctx = context or N.default_context()
        self.k, self.m, self.S, self.batch, self.device = k, m, None, batch, device
        self.sizes = [int(s) for s in sizes]
        self.handle = None
        flags = (ctypes.c_uint8 * max(1, batch * n))(*[1 if f else 0 for r in rows for f in r])
        szs = (ctypes.c_size_t * max(1, batch))(*self.sizes)
        arr = lambda p: (ctypes.c_void_p * max(1, len(p)))(*[int(x) or None for x in p])  # noqa: E731
        h = ctypes.c_void_p()
        bits = (N.RS_DECODE_IDX_STORE if store else 0) | (N.RS_DECODE_CHECK_FINAL if final else 0)
        N.check(N.lib.rs_plan_create_decode_check(self.ctx.handle, device, k, m, batch, szs, flags,
                                                  arr(input_ptrs), arr(dst_ptrs), arr(check_ptrs), bits,
                                                  ctypes.byref(h)),
                "rs_plan_create_decode_check")
        self.handle = h
        return self

    @classmethod
    def decode_repair(cls, k: int, m: int, sizes: Sequence[int], expect, input_ptrs, dst_ptrs, check_ptrs,
                      fix_ptrs=None, store: bool = False, device: int = 0,
                      context: Optional[N.Context] = None) -> "Plan":
        """rs_plan_create_decode_repair: a final decode_check plan whose launch
        names the corrupt shard of a mismatching byte column from the finished check rows, repairs
        the wanted rows within the launch and XORs the error values into the fix buffers.
        fix_ptrs: batch*(k+m) device pointers (None: none), nonzero at expected or compared
        indices only; a zeroed buffer ends as the shard's error row, the shard as delivered ends
        restored (fix may be the input itself). Needs three check rows for a verdict; a stripe has
        at most 16 rows. blame() reads and clears the per-shard column counts, corrupt_stripes()
        the stripes that had a mismatch, repaired or not. A merge launch with wanted rows is NOT
        idempotent."""
        batch = len(sizes)
        n = k + m
        rows = _mask_rows(expect)
        if rows is None or len(rows) != batch or any(len(r) != n for r in rows):
            raise ValueError("expect: batch rows of k+m flags")
        if fix_ptrs is None:
            fix_ptrs = [0] * (batch * n)
        if any(len(p) != batch * n for p in (input_ptrs, dst_ptrs, check_ptrs, fix_ptrs)):
            raise ValueError("need batch*(k+m) input, dst, check and fix pointers each")
        self = cls.__new__(cls)
        self.ctx = context or N.default_context()
        self.k, self.m, self.S, self.batch, self.device = k, m, None, batch, device
        self.sizes = [int(s) for s in sizes]
        self.handle = None
        flags = (ctypes.c_uint8 * max(1, batch * n))(*[1 if f else 0 for r in rows for f in r])
        szs = (ctypes.c_size_t * max(1, batch))(*self.sizes)
        arr = lambda p: (ctypes.c_void_p * max(1, len(p)))(*[int(x) or None for x in p])  # noqa: E731
        h = ctypes.c_void_p()
        N.check(N.lib.rs_plan_create_decode_repair(self.ctx.handle, device, k, m, batch, szs, flags,
                                                   arr(input_ptrs), arr(dst_ptrs), arr(check_ptrs),
                                                   arr(fix_ptrs), N.RS_DECODE_IDX_STORE if store else 0,
                                                   ctypes.byref(h)),
                "rs_plan_create_decode_repair")
        self.handle = h
        return self

    @property
    def bytes(self) -> int:
        """Algorithmic HBM bytes one launch moves."""
        return int(N.lib.rs_plan_bytes(self.handle))

    def launch(self, stream: Optional[torch.cuda.Stream] = None, events=None) -> None:
        """rs_plan_launch; events = (start, stop) torch.cuda.Event pair (timing enabled,
        recorded at least once so the HIP events exist): rs_plan_launch_timed, the
        first kernel dispatch records start when it starts and the last records stop when
        it ends, so start.elapsed_time(stop) is the kernels' own time."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if events is None:
            N.check(N.lib.rs_plan_launch(self.handle, ctypes.c_void_p(s.cuda_stream)),
                    "rs_plan_launch")
            return
        h = [ctypes.c_void_p(e.cuda_event) for e in events]
        if not all(x.value for x in h):
            raise ValueError("record each event once before timing launches with it")
        N.check(N.lib.rs_plan_launch_timed(self.handle, ctypes.c_void_p(s.cuda_stream), *h),
                "rs_plan_launch_timed")

    CEILINGS = {"nolookup": 0, "read": 1, "write": 2, "write64": 3, "write128": 4,
                "write256": 5, "read64": 6, "read128": 7, "read256": 8}

    def launch_ceiling(self, mode: str = "read",
                       stream: Optional[torch.cuda.Stream] = None, events=None) -> None:
        """rs_plan_launch_ceiling (measurement only): this plan's read / write streams
        alone, same grid and tile order ("write" leaves junk in the written shards). The
        A/B build (CALLFS_RS_LIB) adds "nolookup" (the kernel's no-lookup form) and the
        aligned-window probes; the product refuses them (RS_E_ARG). events: as for launch()."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if events is None:
            N.check(N.lib.rs_plan_launch_ceiling(self.handle, ctypes.c_void_p(s.cuda_stream),
                                                 self.CEILINGS[mode]), "rs_plan_launch_ceiling")
            return
        h = [ctypes.c_void_p(e.cuda_event) for e in events]
        if not all(x.value for x in h):
            raise ValueError("record each event once before timing launches with it")
        N.check(N.lib.rs_plan_launch_ceiling_timed(self.handle, ctypes.c_void_p(s.cuda_stream),
                                                   self.CEILINGS[mode], *h),
                "rs_plan_launch_ceiling_timed")

    # tile orders (RS_ORDER_*); on misaligned shards 0..6 name the plain kernel with
    # unaligned accesses and "realign*" the kernel that aligns loads and stores
    ORDER_NAMES = {-1: "none", 0: "consecutive", 1: "g8", 2: "g2", 3: "q8", 4: "q16", 5: "x8",
                   6: "x32", 32: "realign", 37: "realign-x8", 38: "realign-x32",
                   64: "wix", 65: "wix-g8", 66: "wix-g2", 67: "wix-q8", 68: "wix-q16",
                   69: "wix-x8", 70: "wix-x32", 96: "tri", 98: "tri-g2", 99: "tri-q8",
                   100: "tri-q16", 101: "tri-x8", 102: "tri-x32", 128: "realign-tri", 133: "realign-tri-x8",
                   134: "realign-tri-x32", 160: "realign64", 165: "realign64-x8",
                   166: "realign64-x32", 192: "dma", 194: "dma-g2", 195: "dma-q8",
                   198: "dma-x32", 224: "tridb-g4", 225: "tridb-g8", 256: "bs", 257: "bs-g8",
                   258: "bs-g2", 259: "bs-q8", 260: "bs-q16", 261: "bs-x8", 262: "bs-x32",
                   512: "mixed", 1024: "ragged", 2048: "required", 4096: "update",
                   8192: "locate", 16384: "correct", 32768: "decode-idx",
                   65536: "decode-check", 131072: "decode-repair"}

    def tune(self, reps: int = 5, stream: Optional[torch.cuda.Stream] = None) -> list:
        """rs_plan_tune: time each launch group in every tile order its kernel offers
        and keep the fastest for later launches (synchronous; outputs recomputed to the
        same bytes). Returns the chosen order name per launch group."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        n = int(N.lib.rs_plan_groups(self.handle))  # one entry per launch group
        orders = (ctypes.c_int * n)()
        N.check(N.lib.rs_plan_tune(self.handle, ctypes.c_void_p(s.cuda_stream), reps, orders, n),
                "rs_plan_tune")
        return [self.ORDER_NAMES.get(orders[i], str(orders[i])) for i in range(n)]

    def set_orders(self, names: Sequence[str]) -> None:
        """rs_plan_set_orders: pin launch group i to tile order names[i] ("none" = the
        rule). An order the group's kernel does not offer raises NativeError (RS_E_ARG)
        and leaves the plan unchanged."""
        codes = {v: k for k, v in self.ORDER_NAMES.items()}
        arr = (ctypes.c_int * len(names))(*[codes[nm] for nm in names])
        N.check(N.lib.rs_plan_set_orders(self.handle, arr, len(names)), "rs_plan_set_orders")

    def forms(self) -> list:
        """rs_plan_forms: the kernel form (order name) each launch group of the next launch
        runs: the pinned or tuned order, else the rule's ("bs-*" once the rule's bit-sliced
        kernel is compiled)."""
        n = int(N.lib.rs_plan_groups(self.handle))
        out = (ctypes.c_int * max(n, 1))()
        got = N.lib.rs_plan_forms(self.handle, out, n)
        if got < 0:
            N.check(got, "rs_plan_forms")
        return [self.ORDER_NAMES.get(out[i], str(out[i])) for i in range(n)]

    def corrupt(self, stream: Optional[torch.cuda.Stream] = None) -> bool:
        """Synchronises the stream; True when a Verify row mismatched (then clears)."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        c = ctypes.c_int(0)
        N.check(N.lib.rs_plan_status(self.handle, ctypes.c_void_p(s.cuda_stream),
                                     ctypes.byref(c)), "rs_plan_status")
        return bool(c.value)

    def corrupt_stripes(self, stream: Optional[torch.cuda.Stream] = None) -> list:
        """Synchronises the stream; indices of the stripes whose Verify rows mismatched
        since the last status call (then clears)."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        flags = (ctypes.c_int * self.batch)()
        N.check(N.lib.rs_plan_stripe_status(self.handle, ctypes.c_void_p(s.cuda_stream), flags),
                "rs_plan_stripe_status")
        return [b for b in range(self.batch) if flags[b]]

    def close(self) -> None:
        if getattr(self, "handle", None):
            N.lib.rs_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Feed:
    """rs_feed_create / rs_feed_launch: one stripe of S-byte shards whose k
    expected, wanted and compared shards are fixed up front; every launch delivers one shard into
    the resident rows. expect: k+m flags, exactly k set. dst, check: k+m device pointers, nonzero =
    shard i is wanted / compared and this is its S-byte accumulator (neither at an expected index,
    never both at one). At most 16 rows. The tables are built and uploaded once, here."""

    def __init__(self, k: int, m: int, S: int, expect, dst, check, device: int = 0,
                 context: Optional[N.Context] = None):
        self.ctx = context or N.default_context()
        n = k + m
        if len(expect) != n or len(dst) != n or len(check) != n:
            raise ValueError("need k+m expect flags, dst pointers and check pointers")
        self.k, self.m, self.S, self.device = k, m, S, device
        self.handle = None
        flags = (ctypes.c_uint8 * n)(*[1 if f else 0 for f in expect])
        arr = lambda p: (ctypes.c_void_p * n)(*[int(x) or None for x in p])  # noqa: E731
        h = ctypes.c_void_p()
        N.check(N.lib.rs_feed_create(self.ctx.handle, device, k, m, S, flags, arr(dst), arr(check),
                                     ctypes.byref(h)), "rs_feed_create")
        self.handle = h

    def launch(self, idx: int, src: int, store: bool = False,
               stream: Optional[torch.cuda.Stream] = None) -> None:
        """Delivers shard idx (expected or compared) from `src`, the address of S bytes the device
        can read, at any alignment: every row ^= its coefficient times the shard, or = with
        store=True (no row is read, every row is written). Only enqueues. A merge launch is NOT
        idempotent."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        N.check(N.lib.rs_feed_launch(self.handle, idx, ctypes.c_void_p(int(src)),
                                     N.RS_DECODE_IDX_STORE if store else 0,
                                     ctypes.c_void_p(s.cuda_stream)), "rs_feed_launch")

    def close(self) -> None:
        if getattr(self, "handle", None):
            N.lib.rs_feed_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Absorb:
    """rs_absorb_create / rs_absorb_launch: the m parity rows of one object of k
    data shards of S bytes, resident on the device; every launch folds one byte range of the
    object's body in. rows: m device pointers to S-byte accumulators, zero before the first
    launch. At most 16 rows. The tables are built and uploaded once, here."""

    def __init__(self, k: int, m: int, S: int, rows, device: int = 0,
                 context: Optional[N.Context] = None):
        self.ctx = context or N.default_context()
        if len(rows) != m:
            raise ValueError("need m row pointers")
        self.k, self.m, self.S, self.device = k, m, S, device
        self.handle = None
        arr = (ctypes.c_void_p * m)(*[int(x) or None for x in rows])
        h = ctypes.c_void_p()
        N.check(N.lib.rs_absorb_create(self.ctx.handle, device, k, m, S, arr, ctypes.byref(h)),
                "rs_absorb_create")
        self.handle = h

    def launch(self, off: int, length: int, src: int,
               stream: Optional[torch.cuda.Stream] = None) -> None:
        """Folds body bytes [off, off + length) in from `src`, the address of `length` bytes the
        device can read, at any alignment: row j ^= P[j][i] * byte for every byte (shard i, column
        c) of the range, at column c. Only enqueues one kernel. NOT idempotent: every body byte
        is fed exactly once."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        N.check(N.lib.rs_absorb_launch(self.handle, off, length, ctypes.c_void_p(int(src)),
                                       ctypes.c_void_p(s.cuda_stream)), "rs_absorb_launch")

    def close(self) -> None:
        if getattr(self, "handle", None):
            N.lib.rs_absorb_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HashPlan:
    """Batched SHA-256 (erasure.ShardChecksum, codec.go:81-84) of device-resident
    messages: rs_sha256_plan_* over `pointers`/`lengths` (device addresses, bytes)."""

    def __init__(self, pointers: Sequence[int], lengths: Sequence[int], device: int = 0,
                 context: Optional[N.Context] = None):
        self.ctx = context or N.default_context()
        if len(pointers) != len(lengths):
            raise ValueError("pointers/lengths length mismatch")
        self.count = len(pointers)
        self.device = device
        ptrs = (ctypes.c_void_p * max(1, self.count))(*pointers)
        lens = (ctypes.c_uint64 * max(1, self.count))(*lengths)
        h = ctypes.c_void_p()
        N.check(N.lib.rs_sha256_plan_create(self.ctx.handle, device, ptrs, lens, self.count,
                                            ctypes.byref(h)), "rs_sha256_plan_create")
        self.handle = h

    def launch(self, digests: torch.Tensor, stream: Optional[torch.cuda.Stream] = None) -> None:
        """digests: uint8 CUDA tensor of at least 32*count bytes (4-B aligned)."""
        if digests.dtype != torch.uint8 or digests.numel() < 32 * self.count:
            raise ValueError("need a uint8 tensor of 32*count bytes")
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        N.check(N.lib.rs_sha256_plan_launch(self.handle, ctypes.c_void_p(digests.data_ptr()),
                                            ctypes.c_void_p(s.cuda_stream)), "rs_sha256_plan_launch")

    def hexdigests(self) -> list:
        out = torch.empty(32 * max(1, self.count), dtype=torch.uint8,
                          device=torch.device("cuda", self.device))
        self.launch(out)
        raw = out.cpu().numpy().tobytes()
        return [raw[32 * i:32 * (i + 1)].hex() for i in range(self.count)]

    def close(self) -> None:
        if getattr(self, "handle", None):
            N.lib.rs_sha256_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_checksums(sb: StripeBatch) -> list:
    """ShardChecksum of every shard of a device-resident batch: [stripe][shard] hex."""
    dev = sb.device.index if sb.device.index is not None else 0
    hp = HashPlan(sb.pointers(), [sb.S] * (sb.batch * sb.n), dev)
    flat = hp.hexdigests()
    hp.close()
    return [flat[b * sb.n:(b + 1) * sb.n] for b in range(sb.batch)]
