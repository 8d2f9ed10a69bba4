"""Host-side mirror of CallFS's Go `erasure` codec, backed by the HIP C ABI.

Same names, argument meaning and error behaviour as the reference:

    Go (erasure/)                                   here
    ErasureProfile{DataShards,ParityShards,...}     ErasureProfile(data_shards, parity_shards, shard_size)  metadata.go:4-8
    NewCodec()                                      Codec()                                                  codec.go:15-17
    (*Codec).Encode(data, profile)                  Codec.encode(data, profile) -> list of n shards          codec.go:21-41
    (*Codec).Decode(shards, profile, originalSize)  Codec.decode(shards, profile, original_size) -> bytes    codec.go:45-78
    (no counterpart: many objects per call)         Codec.encode_many / Codec.decode_many                    DESIGN.md §7.6
    ShardChecksum(data)                             shard_checksum(data)                                     codec.go:81-84
    ErrInsufficientShards/ErrShardCorrupted/...     exception classes of the same names                      errors.go:7-10

Go compares the sentinel errors by identity (codec_test.go:113,118); here each
sentinel is an exception class, and the wrapped upstream errors
("erasure: failed to split data: %w", codec.go:33 …) are raised as instances of the
upstream error's class carrying the wrapped message, so `isinstance` plays the role
of errors.Is and str() matches the Go .Error() text.

All shard arithmetic runs on the GPU through libcallfs_rs.so; there is no CPU path.
"""
from __future__ import annotations

import ctypes
import hashlib
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N


# ---- errors (erasure/errors.go:7-10 and the upstream reedsolomon values) -------------

class ErasureError(Exception):
    """Base class for every error this module raises."""

    text = "erasure error"

    def __init__(self, message: Optional[str] = None):
        super().__init__(message if message is not None else self.text)


class ErrInsufficientShards(ErasureError):
    text = "erasure: insufficient shards for reconstruction (code 3050)"


class ErrShardCorrupted(ErasureError):
    text = "erasure: shard checksum mismatch (code 3051)"


class ErrInvalidProfile(ErasureError):
    text = "erasure: invalid erasure profile parameters (code 3054)"


class ErrShardNotFound(ErasureError):
    text = "erasure: shard not found on this node (code 3055)"


class ErrShortData(ErasureError):
    text = "not enough data to fill the number of requested shards"


class ErrTooFewShards(ErasureError):
    text = "too few shards given"


class ErrShardNoData(ErasureError):
    text = "no shard data"


class ErrShardSize(ErasureError):
    text = "shard sizes do not match"


class ErrSingular(ErasureError):
    text = "matrix is singular"


class ErrInvalidInput(ErasureError):
    """upstream Update: a changed shard was given without its old bytes."""

    text = "invalid input"


class ErrInvalidShardIdx(ErasureError):
    """upstream EncodeIdx: the shard index is not a data shard's."""

    text = "invalid shard index"


class ErrUnsupportedProfile(ErasureError):
    """k+m > 256: upstream reedsolomon.New switches to Leopard GF(2^16); the GPU codec
    does not implement it and the Go shim keeps the CPU codec for such profiles."""

    text = "profile needs the GF(2^16) (Leopard) codec: k+m > 256"


_UPSTREAM = {
    N.RS_E_SHORT_DATA: ErrShortData,
    N.RS_E_TOO_FEW_SHARDS: ErrTooFewShards,
    N.RS_E_SHARD_SIZE: ErrShardSize,
    N.RS_E_NO_DATA: ErrShardNoData,
    N.RS_E_SINGULAR: ErrSingular,
    N.RS_E_UNSUPPORTED: ErrUnsupportedProfile,
}


def _wrapped(rc: int, prefix: str) -> Exception:
    """fmt.Errorf(prefix + ": %w", upstreamErr)."""
    cls = _UPSTREAM.get(rc)
    if cls is None:
        return N.NativeError(rc, prefix)
    return cls(f"{prefix}: {cls.text}")


def _check_max_errors(max_errors: int, call: str) -> None:
    """The _ex calls' own argument, with their codes: below 1 RS_E_ARG,
    above 2 RS_E_UNSUPPORTED."""
    if max_errors < 1:
        raise N.NativeError(N.RS_E_ARG, call)
    if max_errors > 2:
        raise N.NativeError(N.RS_E_UNSUPPORTED, call)


def _decode_error(rc: int) -> Exception:
    """What Codec.decode raises for a nonzero code of rs_codec_decode (codec.go:45-78)."""
    if rc == N.RS_E_CORRUPT:
        return ErrShardCorrupted()
    if rc == N.RS_E_INSUFFICIENT:
        return ErrInsufficientShards()
    if rc == N.RS_E_INVALID_PROFILE:
        return ErrInvalidProfile()
    if rc in (N.RS_E_TOO_FEW_SHARDS, N.RS_E_SHARD_SIZE, N.RS_E_NO_DATA, N.RS_E_SINGULAR):
        return _wrapped(rc, "erasure: reconstruction failed")
    return N.NativeError(rc, "erasure: decode")


# ---- profile -----------------------------------------------------------------------

@dataclass
class ErasureProfile:
    """erasure/metadata.go:4-8."""

    data_shards: int
    parity_shards: int
    shard_size: int = 0


def shard_checksum(data) -> str:
    """codec.go:81-84: SHA-256 hex digest of a shard."""
    return hashlib.sha256(bytes(data)).hexdigest()


def shard_layout(data, shards) -> List[tuple]:
    """Where and under which checksum Manager.StoreFile keeps each shard
    (erasure/manager.go:171-184): path ".erasure/<first 8 bytes of SHA-256(object), hex>/<i>"
    and ShardChecksum(shard). The shard files are the raw shard bytes, so files written
    from this codec's shards are what the CPU codec reads back, and the reverse."""
    prefix = hashlib.sha256(bytes(data)).digest()[:8].hex()
    return [(f".erasure/{prefix}/{i}", shard_checksum(sh)) for i, sh in enumerate(shards)]


def _addr(buf) -> int:
    """Address of a bytes-like object's first byte (read-only objects allowed)."""
    a = np.frombuffer(buf, dtype=np.uint8)
    return a.ctypes.data if a.size else 0


def _writable(buf) -> bool:
    return isinstance(buf, (bytearray, np.ndarray)) or (
        isinstance(buf, memoryview) and not buf.readonly)


class Codec:
    """erasure/codec.go:12 Codec — stateless; one instance may be shared by threads
    like the shared *Codec at erasure/manager.go:60."""

    def __init__(self, context: Optional[N.Context] = None):
        self._ctx = context

    @property
    def context(self) -> N.Context:
        if self._ctx is None:
            self._ctx = N.default_context()
        return self._ctx

    def encode(self, data, profile: ErasureProfile) -> List[memoryview]:
        """codec.go:21-41. Returns data_shards+parity_shards equal-length shards: S =
        ceil(len/k); like upstream Split the full data shards are views into `data`
        (no copy), the shard holding the end of the object and any after it are
        zero-padded copies, and only the m parity shards are computed (rs_encode).
        Upstream Split also reuses a Go slice's spare capacity past len for the padded
        and parity shards; Python buffers expose no such capacity, so this mirror always
        allocates them (the Go shim, go/erasure/codec_rocm.go split, does reuse it)."""
        k, m = profile.data_shards, profile.parity_shards
        if k < 1 or m < 1:
            raise ErrInvalidProfile()
        src = memoryview(data).cast("B")
        L = len(src)
        # upstream New succeeds for k+m > 256 (Leopard GF(2^16)), so an empty object
        # still fails in Split first (codec.go:26 then :31)
        if L == 0:
            raise ErrShortData(f"erasure: failed to split data: {ErrShortData.text}")
        if k + m > 256:
            raise _wrapped(N.RS_E_UNSUPPORTED, "erasure: failed to create encoder")
        S = (L + k - 1) // k
        full = L // S  # data shards lying entirely inside `data`
        tail = bytearray(S * (k - full))
        tail[: L - full * S] = src[full * S:]
        parity = bytearray(S * m)
        tv, pv = memoryview(tail), memoryview(parity)
        shards = [src[i * S:(i + 1) * S] for i in range(full)]
        shards += [tv[i * S:(i + 1) * S] for i in range(k - full)]
        shards += [pv[j * S:(j + 1) * S] for j in range(m)]
        dptr = (ctypes.c_void_p * k)(*[_addr(s) for s in shards[:k]])
        pptr = (ctypes.c_void_p * m)(*[_addr(s) for s in shards[k:]])
        rc = N.lib.rs_encode(self.context.handle, k, m, S, dptr, pptr)
        if rc != N.RS_OK:
            raise _wrapped(rc, "erasure: failed to encode parity")
        return shards

    def decode(self, shards: List, profile: ErasureProfile, original_size: int,
               data_only: bool = False) -> bytearray:
        """codec.go:45-78. `None` or empty entries are missing shards; they are
        reconstructed in place (the list is mutated, as Go mutates its [][]byte).
        Returns a fresh buffer of original_size bytes (Go: buf[:originalSize]).
        data_only: rs_codec_decode_data (upstream ReconstructData in Reconstruct's place):
        the same bytes and errors, but missing parity shards are not rebuilt and stay None."""
        k, m = profile.data_shards, profile.parity_shards
        if k < 1 or m < 1:
            raise ErrInvalidProfile()
        n = k + m
        if k + m > 256:
            raise _wrapped(N.RS_E_UNSUPPORTED, "erasure: failed to create decoder")
        if len(shards) != n:
            raise ErrTooFewShards(f"erasure: reconstruction failed: {ErrTooFewShards.text}")
        lens = (ctypes.c_size_t * n)()
        for i, s in enumerate(shards):
            lens[i] = 0 if s is None else len(s)
        S = next((lens[i] for i in range(n) if lens[i]), 0)
        bufs = list(shards)
        for i in range(n):
            if lens[i] == 0 and S and (i < k or not data_only):
                bufs[i] = bytearray(S)  # upstream Reconstruct allocates missing shards
        ptrs = (ctypes.c_void_p * n)(*[_addr(b) if b is not None and len(b) else 0
                                      for b in bufs])
        out = bytearray(max(int(original_size), 0))
        fn = N.lib.rs_codec_decode_data if data_only else N.lib.rs_codec_decode
        rc = fn(self.context.handle, k, m, ptrs, lens, _addr(out) if out else None,
                int(original_size))
        # upstream Reconstruct (codec.go:55) has filled the nil entries before Verify
        # (:59) and the join-length check (:73) can fail, so ErrShardCorrupted and
        # ErrInsufficientShards leave them filled too (as the Go shim does)
        if rc in (N.RS_OK, N.RS_E_CORRUPT, N.RS_E_INSUFFICIENT):
            for i in range(n):
                if (shards[i] is None or len(shards[i]) == 0) and lens[i]:
                    shards[i] = bufs[i]
        if rc == N.RS_OK:
            return out
        raise _decode_error(rc)

    def decode_session(self, profile: ErasureProfile, original_size: int, expect: Sequence[int],
                       compare: Sequence[int] = (), repair: bool = False) -> "ObjectDecodeSession":
        """A progressive decode for a download that receives its shards one at
        a time, Manager.RetrieveFile's case: expect names the k shard indices that will be fed,
        compare the indices fetched beyond them that are checked against them (with repair=True:
        and used to repair a corrupt one). feed(idx, shard) as each lands, from any thread;
        finish() returns the object's original_size bytes, bit for bit what decode returns for
        the same shards. The data shards outside expect are the ones rebuilt."""
        k, m = profile.data_shards, profile.parity_shards
        if k < 1 or m < 1:
            raise ErrInvalidProfile()
        if k + m > 256:
            raise _wrapped(N.RS_E_UNSUPPORTED, "erasure: failed to create decoder")
        n = k + m
        size = max(int(original_size), 0)
        S = max(1, (size + k - 1) // k)
        e, c = set(int(i) for i in expect), set(int(i) for i in compare)
        if any(i < 0 or i >= n for i in e | c):
            raise ErrInvalidShardIdx()
        session = DecodeSession(k, m, S, [i in e for i in range(n)],
                                [i < k and i not in e and i not in c for i in range(n)],
                                [i in c for i in range(n)], repair, self.context)
        return ObjectDecodeSession(session, size)

    def encode_session(self, profile: ErasureProfile, size: int) -> "ObjectEncodeSession":
        """A progressive encode for an upload whose body arrives in pieces,
        Manager.StoreFile's case with the request body read as it comes: feed(off, data) or
        write(data) each piece, from any thread, every byte exactly once; finish() returns the
        shards, bit for bit what encode returns for the whole body. Errors as encode."""
        k, m = profile.data_shards, profile.parity_shards
        if k < 1 or m < 1:
            raise ErrInvalidProfile()
        if int(size) <= 0:
            raise ErrShortData(f"erasure: failed to split data: {ErrShortData.text}")
        if k + m > 256:
            raise _wrapped(N.RS_E_UNSUPPORTED, "erasure: failed to create encoder")
        return ObjectEncodeSession(EncodeSession(k, m, int(size), self.context))

    def decode_heal(self, shards: List, profile: ErasureProfile,
                    original_size: int, max_errors: int = 1) -> Tuple[bytearray, List[int]]:
        """rs_codec_decode_heal: decode() that repairs what it can where
        decode() raises ErrShardCorrupted. The corrupt shards are located from the parity
        syndromes; when they explain every mismatching column and a compared shard is left
        to confirm with, they are rebuilt in place (writable buffers) with the missing ones.
        Returns (data, healed shard indices); every other error is decode()'s.
        max_errors=2 (rs_codec_decode_heal_ex, §5.12.1) also heals two shards that are
        corrupt in the same byte columns, where four or more shards are compared."""
        k, m = profile.data_shards, profile.parity_shards
        if k < 1 or m < 1:
            raise ErrInvalidProfile()
        n = k + m
        if k + m > 256:
            raise _wrapped(N.RS_E_UNSUPPORTED, "erasure: failed to create decoder")
        _check_max_errors(max_errors, "rs_codec_decode_heal_ex")
        if len(shards) != n:
            raise ErrTooFewShards(f"erasure: reconstruction failed: {ErrTooFewShards.text}")
        lens = (ctypes.c_size_t * n)()
        for i, s in enumerate(shards):
            lens[i] = 0 if s is None else len(s)
        S = next((lens[i] for i in range(n) if lens[i]), 0)
        bufs = list(shards)
        for i in range(n):
            if lens[i] == 0 and S:
                bufs[i] = bytearray(S)
            elif lens[i] and not _writable(bufs[i]):
                raise TypeError("decode_heal rebuilds corrupt shards in place: writable buffers")
        ptrs = (ctypes.c_void_p * n)(*[_addr(b) if b is not None and len(b) else 0
                                      for b in bufs])
        out = bytearray(max(int(original_size), 0))
        healed = (ctypes.c_uint8 * n)()
        rc = N.lib.rs_codec_decode_heal_ex(self.context.handle, k, m, ptrs, lens,
                                           _addr(out) if out else None, int(original_size), healed,
                                           int(max_errors))
        if rc in (N.RS_OK, N.RS_E_CORRUPT, N.RS_E_INSUFFICIENT):
            for i in range(n):
                if (shards[i] is None or len(shards[i]) == 0) and lens[i]:
                    shards[i] = bufs[i]
        if rc == N.RS_OK:
            return out, [i for i in range(n) if healed[i]]
        raise _decode_error(rc)

    def decode_correct(self, shards: List, profile: ErasureProfile,
                       original_size: int) -> Tuple[bytearray, List[int]]:
        """rs_codec_decode_correct: decode() after one correct() over the
        present shards (writable buffers): in a stripe that compares three or more shards, every
        byte column with one corrupt byte is repaired in place, however many shards the damage
        is spread over. Returns (data, indices of the shards that had bytes corrected); raises
        ErrShardCorrupted exactly when decode() still does after the correction. Every other
        error is decode()'s."""
        k, m = profile.data_shards, profile.parity_shards
        if k < 1 or m < 1:
            raise ErrInvalidProfile()
        n = k + m
        if k + m > 256:
            raise _wrapped(N.RS_E_UNSUPPORTED, "erasure: failed to create decoder")
        if len(shards) != n:
            raise ErrTooFewShards(f"erasure: reconstruction failed: {ErrTooFewShards.text}")
        lens = (ctypes.c_size_t * n)()
        for i, s in enumerate(shards):
            lens[i] = 0 if s is None else len(s)
        S = next((lens[i] for i in range(n) if lens[i]), 0)
        bufs = list(shards)
        for i in range(n):
            if lens[i] == 0 and S:
                bufs[i] = bytearray(S)
            elif lens[i] and not _writable(bufs[i]):
                raise TypeError("decode_correct repairs corrupt bytes in place: writable buffers")
        ptrs = (ctypes.c_void_p * n)(*[_addr(b) if b is not None and len(b) else 0
                                      for b in bufs])
        out = bytearray(max(int(original_size), 0))
        corrected = (ctypes.c_uint8 * n)()
        rc = N.lib.rs_codec_decode_correct(self.context.handle, k, m, ptrs, lens,
                                           _addr(out) if out else None, int(original_size), corrected)
        if rc in (N.RS_OK, N.RS_E_CORRUPT, N.RS_E_INSUFFICIENT):
            for i in range(n):
                if (shards[i] is None or len(shards[i]) == 0) and lens[i]:
                    shards[i] = bufs[i]
        if rc == N.RS_OK:
            return out, [i for i in range(n) if corrected[i]]
        raise _decode_error(rc)

    def encode_many(self, datas: Sequence, profile: ErasureProfile
                    ) -> Tuple[List[Optional[List[memoryview]]], List[Optional[Exception]]]:
        """Codec.encode for many objects of one profile in one native call
        (rs_codec_encode_batch: one pipeline over all of them, Split done on the way into its
        staging). Returns (shards_per_object, errors): errors[b] is None and
        shards_per_object[b] the n shards of object b (views into one fresh n*S buffer), or
        errors[b] is an instance of the class and message encode() would have raised for that
        object and shards_per_object[b] is None. Profile errors raise."""
        k, m = profile.data_shards, profile.parity_shards
        if k < 1 or m < 1:
            raise ErrInvalidProfile()
        if k + m > 256:
            raise _wrapped(N.RS_E_UNSUPPORTED, "erasure: failed to create encoder")
        n, B = k + m, len(datas)
        srcs = [memoryview(d).cast("B") for d in datas]
        outs = [bytearray(n * ((len(s) + k - 1) // k)) for s in srcs]
        lens = (ctypes.c_size_t * max(B, 1))(*[len(s) for s in srcs])
        caps = (ctypes.c_size_t * max(B, 1))(*[len(o) for o in outs])
        sizes = (ctypes.c_size_t * max(B, 1))()
        status = (ctypes.c_int * max(B, 1))()
        rc = N.lib.rs_codec_encode_batch(self.context.handle, k, m, B, _shard_ptrs(srcs or [None]),
                                         lens, _shard_ptrs(outs or [None]), caps, sizes, status)
        st = list(status)[:B]
        if rc != N.RS_OK and rc not in st:
            raise N.NativeError(rc, "rs_codec_encode_batch")  # call-level
        shards, errors = [], []
        for b in range(B):
            if st[b] == N.RS_OK:
                S, mv = sizes[b], memoryview(outs[b])
                shards.append([mv[i * S:(i + 1) * S] for i in range(n)])
                errors.append(None)
                continue
            shards.append(None)
            errors.append(_wrapped(st[b], "erasure: failed to split data"
                                   if st[b] == N.RS_E_SHORT_DATA else "erasure: failed to encode parity"))
        return shards, errors

    def decode_many(self, shards_per_object: Sequence[List], profile: ErasureProfile,
                    original_sizes: Sequence[int], data_only: bool = False
                    ) -> Tuple[List[Optional[bytearray]], List[Optional[Exception]]]:
        """Codec.decode for many objects of one profile in one native call
        (rs_codec_decode_batch: Reconstruct, Verify and the join / trim of every object in one
        pipeline). Returns (objects, errors): errors[b] is None and objects[b] the
        original_sizes[b] bytes of object b, or errors[b] is an instance of the class and
        message decode() would have raised for that object and objects[b] is None. Each shard
        list is mutated as decode() mutates it. Profile errors raise.
        data_only: rs_codec_decode_data_batch, as decode(data_only=True) per object."""
        k, m = profile.data_shards, profile.parity_shards
        if k < 1 or m < 1:
            raise ErrInvalidProfile()
        n = k + m
        if n > 256:
            raise _wrapped(N.RS_E_UNSUPPORTED, "erasure: failed to create decoder")
        if len(original_sizes) != len(shards_per_object):
            raise ValueError("one original size per object")
        B = len(shards_per_object)
        errors: List[Optional[Exception]] = [None] * B
        run = []  # the objects handed to the native call
        for b, shards in enumerate(shards_per_object):
            if len(shards) != n:
                errors[b] = ErrTooFewShards(f"erasure: reconstruction failed: {ErrTooFewShards.text}")
            elif int(original_sizes[b]) < 0:
                errors[b] = N.NativeError(N.RS_E_ARG, "erasure: decode")
            else:
                run.append(b)
        R = len(run)
        lens = (ctypes.c_size_t * max(R * n, 1))()
        flat, bufs, outs = [], [], []
        for j, b in enumerate(run):
            shards = shards_per_object[b]
            ln = [0 if s is None else len(s) for s in shards]
            S = next((x for x in ln if x), 0)
            cp = list(shards)
            for i in range(n):
                lens[j * n + i] = ln[i]
                if ln[i] == 0 and S and (i < k or not data_only):
                    cp[i] = bytearray(S)  # upstream Reconstruct allocates missing shards
            bufs.append(cp)
            flat += cp
            outs.append(bytearray(int(original_sizes[b])))
        sizes = (ctypes.c_int64 * max(R, 1))(*[int(original_sizes[b]) for b in run])
        status = (ctypes.c_int * max(R, 1))()
        fn = N.lib.rs_codec_decode_data_batch if data_only else N.lib.rs_codec_decode_batch
        rc = fn(self.context.handle, k, m, R, _shard_ptrs(flat or [None]), lens,
                _shard_ptrs(outs or [None]), sizes, status)
        st = list(status)[:R]
        if rc != N.RS_OK and rc not in st:
            raise N.NativeError(rc, "rs_codec_decode_batch")  # call-level
        objects: List[Optional[bytearray]] = [None] * B
        for j, b in enumerate(run):
            shards = shards_per_object[b]
            if st[j] in (N.RS_OK, N.RS_E_CORRUPT, N.RS_E_INSUFFICIENT):
                for i in range(n):
                    if (shards[i] is None or len(shards[i]) == 0) and lens[j * n + i]:
                        shards[i] = bufs[j][i]
            if st[j] == N.RS_OK:
                objects[b] = outs[j]
            else:
                errors[b] = _decode_error(st[j])
        return objects, errors

    def encode_many_sums(self, datas: Sequence, profile: ErasureProfile
                         ) -> Tuple[List[Optional[List[memoryview]]], List[Optional[List[str]]],
                                    List[Optional[Exception]]]:
        """encode_many with every shard's checksum taken on the way through the pipeline
        (rs_codec_encode_batch_sums): what Manager.StoreFile computes with
        ShardChecksum beside Codec.Encode. Returns (shards_per_object, checksums_per_object,
        errors): checksums_per_object[b][i] is the 64-character hex string shard_checksum()
        returns for shard i of object b, or None where errors[b] is set."""
        k, m = profile.data_shards, profile.parity_shards
        if k < 1 or m < 1:
            raise ErrInvalidProfile()
        if k + m > 256:
            raise _wrapped(N.RS_E_UNSUPPORTED, "erasure: failed to create encoder")
        n, B = k + m, len(datas)
        srcs = [memoryview(d).cast("B") for d in datas]
        outs = [bytearray(n * ((len(s) + k - 1) // k)) for s in srcs]
        lens = (ctypes.c_size_t * max(B, 1))(*[len(s) for s in srcs])
        caps = (ctypes.c_size_t * max(B, 1))(*[len(o) for o in outs])
        sizes = (ctypes.c_size_t * max(B, 1))()
        status = (ctypes.c_int * max(B, 1))()
        digests = bytearray(max(B, 1) * n * 32)
        rc = N.lib.rs_codec_encode_batch_sums(self.context.handle, k, m, B, _shard_ptrs(srcs or [None]),
                                              lens, _shard_ptrs(outs or [None]), caps, sizes,
                                              _addr(digests), status)
        st = list(status)[:B]
        if rc != N.RS_OK and rc not in st:
            raise N.NativeError(rc, "rs_codec_encode_batch_sums")  # call-level
        shards, sums, errors = [], [], []
        for b in range(B):
            if st[b] == N.RS_OK:
                S, mv = sizes[b], memoryview(outs[b])
                shards.append([mv[i * S:(i + 1) * S] for i in range(n)])
                sums.append([digests[(b * n + i) * 32:(b * n + i + 1) * 32].hex() for i in range(n)])
                errors.append(None)
                continue
            shards.append(None)
            sums.append(None)
            errors.append(_wrapped(st[b], "erasure: failed to split data"
                                   if st[b] == N.RS_E_SHORT_DATA else "erasure: failed to encode parity"))
        return shards, sums, errors

    def decode_many_sums(self, shards_per_object: Sequence[List], checksums_per_object: Sequence[Sequence],
                         profile: ErasureProfile, original_sizes: Sequence[int]
                         ) -> Tuple[List[Optional[bytearray]], List[List[int]], List[Optional[Exception]]]:
        """decode_many with every present shard checked against its recorded checksum on the
        way through the pipeline (rs_codec_decode_batch_sums): what
        Manager.RetrieveFile does before Codec.Decode (manager.go:283-296). A present shard
        whose SHA-256 differs from checksums_per_object[b][i] (hex, as shard_checksum() gives
        it; entries of missing shards are ignored and may be None) counts as missing: it is
        rebuilt in place (a writable buffer), the rest is verified and the object joined.
        Returns (objects, bad_indices, errors): bad_indices[b] lists the shards of object b that
        failed their checksum; errors[b] is what decode() would raise for the object with
        those shards missing."""
        k, m = profile.data_shards, profile.parity_shards
        if k < 1 or m < 1:
            raise ErrInvalidProfile()
        n = k + m
        if n > 256:
            raise _wrapped(N.RS_E_UNSUPPORTED, "erasure: failed to create decoder")
        if len(original_sizes) != len(shards_per_object) or len(checksums_per_object) != len(shards_per_object):
            raise ValueError("one original size and one checksum list per object")
        B = len(shards_per_object)
        errors: List[Optional[Exception]] = [None] * B
        run = []  # the objects handed to the native call
        for b, shards in enumerate(shards_per_object):
            if len(shards) != n:
                errors[b] = ErrTooFewShards(f"erasure: reconstruction failed: {ErrTooFewShards.text}")
            elif int(original_sizes[b]) < 0 or len(checksums_per_object[b]) != n:
                errors[b] = N.NativeError(N.RS_E_ARG, "erasure: decode")
            else:
                run.append(b)
        R = len(run)
        lens = (ctypes.c_size_t * max(R * n, 1))()
        expected = bytearray(max(R, 1) * n * 32)
        flat, bufs, outs = [], [], []
        for j, b in enumerate(run):
            shards = shards_per_object[b]
            ln = [0 if s is None else len(s) for s in shards]
            S = next((x for x in ln if x), 0)
            cp = list(shards)
            for i in range(n):
                lens[j * n + i] = ln[i]
                if ln[i] == 0 and S:
                    cp[i] = bytearray(S)  # upstream Reconstruct allocates missing shards
                elif ln[i]:
                    if not _writable(cp[i]):
                        raise TypeError("decode_many_sums rebuilds a corrupt shard in place: writable buffers")
                    expected[(j * n + i) * 32:(j * n + i + 1) * 32] = bytes.fromhex(checksums_per_object[b][i])
            bufs.append(cp)
            flat += cp
            outs.append(bytearray(int(original_sizes[b])))
        sizes = (ctypes.c_int64 * max(R, 1))(*[int(original_sizes[b]) for b in run])
        status = (ctypes.c_int * max(R, 1))()
        bad = bytearray(max(R, 1) * n)
        rc = N.lib.rs_codec_decode_batch_sums(self.context.handle, k, m, R, _shard_ptrs(flat or [None]), lens,
                                              _addr(expected), _shard_ptrs(outs or [None]), sizes,
                                              _addr(bad), status)
        st = list(status)[:R]
        if rc != N.RS_OK and rc not in st:
            raise N.NativeError(rc, "rs_codec_decode_batch_sums")  # call-level
        objects: List[Optional[bytearray]] = [None] * B
        bad_indices: List[List[int]] = [[] for _ in range(B)]
        for j, b in enumerate(run):
            shards = shards_per_object[b]
            bad_indices[b] = [i for i in range(n) if bad[j * n + i]]
            if st[j] in (N.RS_OK, N.RS_E_CORRUPT, N.RS_E_INSUFFICIENT):
                for i in range(n):
                    if (shards[i] is None or len(shards[i]) == 0) and lens[j * n + i]:
                        shards[i] = bufs[j][i]
            if st[j] == N.RS_OK:
                objects[b] = outs[j]
            else:
                errors[b] = _decode_error(st[j])
        return objects, bad_indices, errors

    def overwrite(self, shards: List, profile: ErasureProfile, offset: int, data) -> None:
        """rs_codec_overwrite: bytes [offset, offset + len(data)) of the object
        whose shards these are (encode's layout: object byte x in data shard x // S at column
        x % S) become `data`. Only the affected parity columns are updated (upstream Update on
        at most three column intervals) and the data shards the range touches are rewritten;
        afterwards `shards` equal encode() of the overwritten object. The touched data shards
        and all parity shards must be writable buffers of one size; the others may be None."""
        k, m = profile.data_shards, profile.parity_shards
        if k < 1 or m < 1:
            raise ErrInvalidProfile()
        if k + m > 256:
            raise _wrapped(N.RS_E_UNSUPPORTED, "erasure: failed to create encoder")
        if len(shards) != k + m:
            raise ErrTooFewShards()
        src = memoryview(data).cast("B")
        S = next((len(s) for s in shards if s is not None and len(s)), 0)
        if any(s is not None and len(s) not in (0, S) for s in shards):
            raise ErrShardSize()
        if S and len(src) and 0 <= offset and offset + len(src) <= k * S:
            touched = list(range(offset // S, (offset + len(src) - 1) // S + 1)) + list(range(k, k + m))
            if not all(shards[i] is not None and _writable(shards[i]) for i in touched):
                raise TypeError("the touched data shards and the parity shards must be writable")
        rc = N.lib.rs_codec_overwrite(self.context.handle, k, m, S, _shard_ptrs(shards), int(offset),
                                      _addr(src) if len(src) else None, len(src))
        if rc != N.RS_OK:
            raise _wrapped(rc, "erasure: failed to update parity")


# ---- reedsolomon.Encoder-level helpers over host shards -----------------------------

def _shard_ptrs(shards: Sequence) -> ctypes.Array:
    return (ctypes.c_void_p * len(shards))(*[_addr(s) if s is not None and len(s) else 0
                                             for s in shards])


def encode_shards(shards: List, k: int, m: int, context: Optional[N.Context] = None) -> None:
    """upstream enc.Encode(shards) (codec.go:36): fills shards[k:] in place. Parity
    entries must be writable buffers of the data shards' size."""
    ctx = context or N.default_context()
    if len(shards) != k + m:
        raise ErrTooFewShards()
    S = len(shards[0])
    if any(len(s) != S for s in shards):
        raise ErrShardSize()
    if not all(_writable(s) for s in shards[k:]):
        raise TypeError("parity shards must be writable")
    data = _shard_ptrs(shards[:k])
    par = _shard_ptrs(shards[k:])
    N.check(N.lib.rs_encode(ctx.handle, k, m, S, data, par), "rs_encode")


def reconstruct(shards: List, k: int, m: int, context: Optional[N.Context] = None) -> None:
    """upstream enc.Reconstruct(shards) (codec.go:55); missing entries are replaced."""
    ctx = context or N.default_context()
    n = k + m
    if len(shards) != n:
        raise ErrTooFewShards()
    lens = (ctypes.c_size_t * n)(*[0 if s is None else len(s) for s in shards])
    S = next((lens[i] for i in range(n) if lens[i]), 0)
    bufs = [bytearray(S) if (lens[i] == 0 and S) else shards[i] for i in range(n)]
    rc = N.lib.rs_reconstruct(ctx.handle, k, m, _shard_ptrs(bufs), lens)
    if rc != N.RS_OK:
        raise _wrapped(rc, "reconstruct")
    for i in range(n):
        if shards[i] is None or len(shards[i]) == 0:
            shards[i] = bufs[i]


def reconstruct_some(shards: List, k: int, m: int, required: Sequence[bool],
                     context: Optional[N.Context] = None) -> None:
    """upstream enc.ReconstructSome(shards, required): only the missing entries whose flag in
    `required` (k+m flags) is set are rebuilt and replaced; the others stay missing."""
    ctx = context or N.default_context()
    n = k + m
    if len(shards) != n:
        raise ErrTooFewShards()
    if len(required) != n:
        raise ValueError("required needs k+m flags")
    lens = (ctypes.c_size_t * n)(*[0 if s is None else len(s) for s in shards])
    S = next((lens[i] for i in range(n) if lens[i]), 0)
    bufs = [bytearray(S) if (lens[i] == 0 and S and required[i]) else shards[i] for i in range(n)]
    req = (ctypes.c_uint8 * n)(*[1 if r else 0 for r in required])
    rc = N.lib.rs_reconstruct_some(ctx.handle, k, m, _shard_ptrs(bufs), lens, req)
    if rc != N.RS_OK:
        raise _wrapped(rc, "reconstruct")
    for i in range(n):
        if (shards[i] is None or len(shards[i]) == 0) and lens[i]:
            shards[i] = bufs[i]


def update(shards: List, new_data: Sequence, k: int, m: int,
           context: Optional[N.Context] = None) -> None:
    """upstream enc.Update(shards, newDatashards): shards holds the old data shards (only
    those that changed are read; the others may be None) and the m parity shards, updated in
    place; new_data has k entries, None = unchanged. The data entries of `shards` are left as
    they are (upstream: "the data shards will remain the same"). A changed shard without its
    old bytes raises ErrInvalidInput, as upstream (the native call's RS_E_ARG)."""
    ctx = context or N.default_context()
    if len(shards) != k + m:
        raise ErrTooFewShards()
    if len(new_data) != k:
        raise ErrTooFewShards()
    changed = [i for i in range(k) if new_data[i] is not None and len(new_data[i])]
    for i in changed:
        if shards[i] is None or len(shards[i]) == 0:
            raise ErrInvalidInput()
    S = next((len(new_data[i]) for i in changed), 0) or next(
        (len(s) for s in shards if s is not None and len(s)), 0)
    if any(len(new_data[i]) != S or len(shards[i]) != S for i in changed) or any(
            s is None or len(s) != S for s in shards[k:]):
        raise ErrShardSize()
    if not all(_writable(s) for s in shards[k:]):
        raise TypeError("parity shards must be writable")
    old = _shard_ptrs([shards[i] if i in changed else None for i in range(k)])
    rc = N.lib.rs_update(ctx.handle, k, m, S, old, _shard_ptrs(list(new_data)), _shard_ptrs(shards[k:]))
    if rc != N.RS_OK:
        raise _wrapped(rc, "update")


def encode_idx(shard, idx: int, parity: List, k: int, m: int,
               context: Optional[N.Context] = None) -> None:
    """upstream enc.EncodeIdx(dataShard, idx, parity): adds data shard idx's contribution to
    the m parity shards in place. Zero the parity before the first shard; the k shards may
    then arrive in any order."""
    ctx = context or N.default_context()
    if not 0 <= idx < k:
        raise ErrInvalidShardIdx()
    if len(parity) != m:
        raise ErrTooFewShards()
    S = len(shard)
    if any(p is None or len(p) != S for p in parity):
        raise ErrShardSize()
    if not all(_writable(p) for p in parity):
        raise TypeError("parity shards must be writable")
    rc = N.lib.rs_encode_idx(ctx.handle, k, m, S, _addr(shard) if S else None, idx, _shard_ptrs(parity))
    if rc != N.RS_OK:
        raise _wrapped(rc, "encode_idx")


def update_batch(old_data: Optional[Sequence[Sequence]], new_data: Sequence[Sequence],
                 parity: Sequence[Sequence], k: int, m: int,
                 context: Optional[N.Context] = None) -> List[int]:
    """rs_update_batch: stripe b has new_data[b] (k entries, None or empty = unchanged), old_data[b] (k
    entries, read where changed) and parity[b] (m writable shards, updated in place). Stripes
    may differ in shard size and in what changed. old_data=None is EncodeIdx mode for the
    whole batch. Returns status[b] (RS_OK, RS_E_NO_DATA, RS_E_ARG)."""
    ctx = context or N.default_context()
    B = len(new_data)
    if len(parity) != B or (old_data is not None and len(old_data) != B):
        raise ValueError("one row of old / new / parity shards per stripe")
    sizes = (ctypes.c_size_t * max(B, 1))()
    for b in range(B):
        if len(new_data[b]) != k or len(parity[b]) != m or (old_data is not None and len(old_data[b]) != k):
            raise ErrTooFewShards()
        ref = [s for s in parity[b] if s is not None]
        S = len(ref[0]) if ref else 0
        rows = list(parity[b]) + [s for s in new_data[b] if s is not None]
        if old_data is not None:
            rows += [old_data[b][i] for i in range(k) if new_data[b][i] is not None and old_data[b][i] is not None]
        if any(s is not None and len(s) != S for s in rows):
            raise ErrShardSize()
        if not all(s is None or _writable(s) for s in parity[b]):
            raise TypeError("parity shards must be writable")
        sizes[b] = S
    def ptrs(rows):
        return _shard_ptrs([s for row in rows for s in row] or [None])

    status = (ctypes.c_int * max(B, 1))()
    rc = N.lib.rs_update_batch(ctx.handle, k, m, B, sizes,
                               None if old_data is None else ptrs(old_data), ptrs(new_data),
                               ptrs(parity), status)
    out = list(status)[:B]
    if rc != N.RS_OK and rc not in out:
        N.check(rc, "rs_update_batch")
    return out


def _decode_idx_rows(dst, expect, inputs, k, m):
    """One stripe's checks for decode_idx / decode_idx_batch: k+m entries each, one shard size
    over every given buffer, writable destinations. Returns that size (0: nothing given)."""
    n = k + m
    if len(dst) != n or len(expect) != n or len(inputs) != n:
        raise ErrTooFewShards()
    given = [s for s in list(dst) + list(inputs) if s is not None]
    S = len(given[0]) if given else 0
    if any(len(s) != S for s in given):
        raise ErrShardSize()
    if not all(s is None or _writable(s) for s in dst):
        raise TypeError("dst shards must be writable")
    return S


def decode_idx(dst: Sequence, expect: Sequence[bool], inputs: Sequence, k: int, m: int,
               store: bool = False, context: Optional[N.Context] = None) -> None:
    """upstream enc.DecodeIdx(dst, expectInput, input): the decode twin of encode_idx. expect
    (k+m flags, exactly k set) fixes the shards the decode will be fed over all calls; inputs
    (k+m entries, None = not delivered with this call) are the shards that have arrived; dst
    (k+m entries, None = not wanted) are writable buffers at indices that are not expected.
    Adds the delivered shards' contribution into every wanted shard, or with store=True stores
    it without reading them. Zero dst before the first call (or store first); once every
    expected shard has been delivered, in any order, dst holds what reconstruct gives from
    those k shards. Fewer than k expected raises ErrTooFewShards; more, an input that is not
    expected or a dst that is raise ErrInvalidInput."""
    ctx = context or N.default_context()
    S = _decode_idx_rows(dst, expect, inputs, k, m)
    ex = (ctypes.c_uint8 * (k + m))(*[1 if e else 0 for e in expect])
    rc = N.lib.rs_decode_idx(ctx.handle, k, m, S, _shard_ptrs(list(dst)), ex, _shard_ptrs(list(inputs)),
                             N.RS_DECODE_IDX_STORE if store else 0)
    if rc == N.RS_E_ARG:
        raise ErrInvalidInput()
    if rc == N.RS_E_INVALID_PROFILE:
        raise ErrInvalidProfile()
    if rc != N.RS_OK:
        raise _wrapped(rc, "decode_idx")


def decode_idx_batch(dst: Sequence[Sequence], expect: Sequence[Sequence[bool]],
                     inputs: Sequence[Sequence], k: int, m: int, store: bool = False,
                     context: Optional[N.Context] = None) -> List[int]:
    """rs_decode_idx_batch: stripe b has dst[b], expect[b] and inputs[b] as decode_idx takes
    them; stripes may differ in shard size, expected set, wanted set and what is delivered.
    Returns status[b] (RS_OK, RS_E_TOO_FEW_SHARDS, RS_E_ARG, RS_E_NO_DATA)."""
    ctx = context or N.default_context()
    B = len(dst)
    if len(expect) != B or len(inputs) != B:
        raise ValueError("one row of dst / expect / input entries per stripe")
    sizes = (ctypes.c_size_t * max(B, 1))()
    for b in range(B):
        sizes[b] = _decode_idx_rows(dst[b], expect[b], inputs[b], k, m)

    def ptrs(rows):
        return _shard_ptrs([s for row in rows for s in row] or [None])

    ex = (ctypes.c_uint8 * max(1, B * (k + m)))(*[1 if e else 0 for row in expect for e in row])
    status = (ctypes.c_int * max(B, 1))()
    rc = N.lib.rs_decode_idx_batch(ctx.handle, k, m, B, sizes, ptrs(dst), ex, ptrs(inputs),
                                   N.RS_DECODE_IDX_STORE if store else 0, status)
    out = list(status)[:B]
    if rc != N.RS_OK and rc not in out:
        N.check(rc, "rs_decode_idx_batch")
    return out


def _decode_check_rows(dst, check, expect, inputs, k, m):
    """_decode_idx_rows with the accumulators: writable, of the stripe's shard size, at indices
    that are not wanted."""
    if len(check) != k + m or len(dst) != k + m:
        raise ErrTooFewShards()
    if any(d is not None and c is not None for d, c in zip(dst, check)):
        raise ErrInvalidInput()
    return _decode_idx_rows([d if d is not None else c for d, c in zip(dst, check)], expect, inputs, k, m)


def _decode_check_bits(store, final):
    return (N.RS_DECODE_IDX_STORE if store else 0) | (N.RS_DECODE_CHECK_FINAL if final else 0)


def decode_check(dst: Sequence, check: Sequence, expect: Sequence[bool], inputs: Sequence, k: int, m: int,
                 store: bool = False, final: bool = False, context: Optional[N.Context] = None) -> None:
    """decode_idx that also checks the shards fetched beyond the k expected ones (DESIGN.md
    §5.15). check (k+m entries, None = not compared) are writable syndrome accumulators at
    indices that are neither expected nor wanted; inputs may then deliver the compared shard
    itself. Every call adds the delivered expected shards' terms, and the compared shard when it
    arrives, into its accumulator (store=True: stores them). final=True writes no accumulator:
    the value it would have received is tested, and a nonzero byte raises ErrShardCorrupted
    after the wanted shards have been written -- what upstream Decode's Verify reports. With
    store=True as well the accumulators are not read: the one-shot decode plus Verify."""
    ctx = context or N.default_context()
    S = _decode_check_rows(dst, check, expect, inputs, k, m)
    ex = (ctypes.c_uint8 * (k + m))(*[1 if e else 0 for e in expect])
    rc = N.lib.rs_decode_check(ctx.handle, k, m, S, _shard_ptrs(list(dst)), _shard_ptrs(list(check)), ex,
                               _shard_ptrs(list(inputs)), _decode_check_bits(store, final))
    if rc == N.RS_E_ARG:
        raise ErrInvalidInput()
    if rc == N.RS_E_INVALID_PROFILE:
        raise ErrInvalidProfile()
    if rc == N.RS_E_CORRUPT:
        raise ErrShardCorrupted()
    if rc != N.RS_OK:
        raise _wrapped(rc, "decode_check")


def decode_check_batch(dst: Sequence[Sequence], check: Sequence[Sequence], expect: Sequence[Sequence[bool]],
                       inputs: Sequence[Sequence], k: int, m: int, store: bool = False, final: bool = False,
                       context: Optional[N.Context] = None) -> List[int]:
    """rs_decode_check_batch: stripe b has dst[b], check[b], expect[b] and inputs[b] as
    decode_check takes them. Returns status[b] (RS_OK, RS_E_TOO_FEW_SHARDS, RS_E_ARG,
    RS_E_NO_DATA, and with final=True RS_E_CORRUPT for a stripe whose compared shards do not
    lie on the expected shards' codeword)."""
    ctx = context or N.default_context()
    B = len(dst)
    if len(check) != B or len(expect) != B or len(inputs) != B:
        raise ValueError("one row of dst / check / expect / input entries per stripe")
    sizes = (ctypes.c_size_t * max(B, 1))()
    for b in range(B):
        sizes[b] = _decode_check_rows(dst[b], check[b], expect[b], inputs[b], k, m)

    def ptrs(rows):
        return _shard_ptrs([s for row in rows for s in row] or [None])

    ex = (ctypes.c_uint8 * max(1, B * (k + m)))(*[1 if e else 0 for row in expect for e in row])
    status = (ctypes.c_int * max(B, 1))()
    rc = N.lib.rs_decode_check_batch(ctx.handle, k, m, B, sizes, ptrs(dst), ptrs(check), ex, ptrs(inputs),
                                     _decode_check_bits(store, final), status)
    out = list(status)[:B]
    if rc != N.RS_OK and rc not in out:
        N.check(rc, "rs_decode_check_batch")
    return out


def _decode_repair_rows(dst, check, fix, expect, inputs, k, m):
    """_decode_check_rows with the fix buffers: k+m entries (None = none), writable, of the
    stripe's shard size."""
    S = _decode_check_rows(dst, check, expect, inputs, k, m)
    if len(fix) != k + m:
        raise ErrTooFewShards()
    if any(f is not None and len(f) != S for f in fix):
        raise ErrShardSize()
    return S


def decode_repair(dst: Sequence, check: Sequence, fix: Sequence, expect: Sequence[bool], inputs: Sequence,
                  k: int, m: int, store: bool = False, context: Optional[N.Context] = None):
    """The final decode_check call that repairs what it flags (rs_decode_repair).
    dst, check, expect and inputs as decode_check takes them; fix (k+m entries, None = none) are
    writable buffers at expected or compared indices into which the shard's error values are
    XORed: a zeroed buffer ends as the error row, the shard as delivered ends restored, and
    fix[i] may be inputs[i] itself when that is writable. Returns the k+m+1 counts: entry i the
    byte columns blamed on shard i, the last the columns left unexplained. With three or more
    compared shards a single corrupt shard per column is repaired in the wanted shards and
    named; any unexplained column raises ErrShardCorrupted after the wanted shards have been
    written, as decode_check does."""
    ctx = context or N.default_context()
    S = _decode_repair_rows(dst, check, fix, expect, inputs, k, m)
    ex = (ctypes.c_uint8 * (k + m))(*[1 if e else 0 for e in expect])
    counts = (ctypes.c_uint64 * (k + m + 1))()
    rc = N.lib.rs_decode_repair(ctx.handle, k, m, S, _shard_ptrs(list(dst)), _shard_ptrs(list(check)),
                                _shard_ptrs(list(fix)), ex, _shard_ptrs(list(inputs)),
                                N.RS_DECODE_IDX_STORE if store else 0, counts)
    if rc == N.RS_E_ARG:
        raise ErrInvalidInput()
    if rc == N.RS_E_INVALID_PROFILE:
        raise ErrInvalidProfile()
    if rc == N.RS_E_CORRUPT:
        raise ErrShardCorrupted()
    if rc != N.RS_OK:
        raise _wrapped(rc, "decode_repair")
    return list(counts)


def decode_repair_batch(dst: Sequence[Sequence], check: Sequence[Sequence], fix: Sequence[Sequence],
                        expect: Sequence[Sequence[bool]], inputs: Sequence[Sequence], k: int, m: int,
                        store: bool = False, context: Optional[N.Context] = None):
    """rs_decode_repair_batch: stripe b has dst[b], check[b], fix[b], expect[b] and inputs[b] as
    decode_repair takes them. Returns (status, counts): status[b] is RS_OK for a clean stripe and
    for one repaired in full, RS_E_CORRUPT where a column is unexplained, or the stripe's own
    refusal; counts[b] its k+m+1 counts."""
    ctx = context or N.default_context()
    B = len(dst)
    if len(check) != B or len(fix) != B or len(expect) != B or len(inputs) != B:
        raise ValueError("one row of dst / check / fix / expect / input entries per stripe")
    sizes = (ctypes.c_size_t * max(B, 1))()
    for b in range(B):
        sizes[b] = _decode_repair_rows(dst[b], check[b], fix[b], expect[b], inputs[b], k, m)

    def ptrs(rows):
        return _shard_ptrs([s for row in rows for s in row] or [None])

    ex = (ctypes.c_uint8 * max(1, B * (k + m)))(*[1 if e else 0 for row in expect for e in row])
    status = (ctypes.c_int * max(B, 1))()
    counts = (ctypes.c_uint64 * max(1, B * (k + m + 1)))()
    rc = N.lib.rs_decode_repair_batch(ctx.handle, k, m, B, sizes, ptrs(dst), ptrs(check), ptrs(fix), ex,
                                      ptrs(inputs), N.RS_DECODE_IDX_STORE if store else 0, status, counts)
    out = list(status)[:B]
    if rc != N.RS_OK and rc not in out:
        N.check(rc, "rs_decode_repair_batch")
    return out, [list(counts[b * (k + m + 1):(b + 1) * (k + m + 1)]) for b in range(B)]


class DecodeSession:
    """rs_session_open: a progressive decode of one stripe whose rows stay on the
    device. expect, want and compare are k+m flags each: the k shards that will be fed, the shards
    to rebuild, the shards fetched beyond the k that are checked against them. feed() delivers one
    shard from host memory, from any thread and in any order; peek() reads a row's partial result;
    finish() closes the decode -- with repair=True it also repairs what the compared shards
    explain. A context manager: leaving it closes the session."""

    def __init__(self, k: int, m: int, S: int, expect: Sequence[bool], want: Sequence[bool],
                 compare: Optional[Sequence[bool]] = None, repair: bool = False,
                 context: Optional[N.Context] = None):
        self.ctx = context or N.default_context()
        n = k + m
        compare = [False] * n if compare is None else compare
        if len(expect) != n or len(want) != n or len(compare) != n:
            raise ErrTooFewShards()
        self.k, self.m, self.S, self.repair = k, m, int(S), repair
        self.want = [bool(w) for w in want]
        self.handle = None
        self.shards: List = [None] * n
        flags = lambda v: (ctypes.c_uint8 * n)(*[1 if f else 0 for f in v])  # noqa: E731
        h = ctypes.c_void_p()
        rc = N.lib.rs_session_open(self.ctx.handle, k, m, self.S, flags(expect), flags(want), flags(compare),
                                   N.RS_SESSION_REPAIR if repair else N.RS_SESSION_CHECK, ctypes.byref(h))
        if rc == N.RS_E_ARG:
            raise ErrInvalidInput()
        if rc == N.RS_E_INVALID_PROFILE:
            raise ErrInvalidProfile()
        if rc != N.RS_OK:
            raise _wrapped(rc, "decode_session")
        self.handle = h

    def feed(self, idx: int, shard) -> None:
        """Delivers shard idx (S bytes), expected or compared, once. Returns when `shard` may be
        reused."""
        if len(shard) != self.S:
            raise ErrShardSize()
        rc = N.lib.rs_session_feed(self.handle, int(idx), ctypes.c_void_p(_addr(shard)))
        if rc == N.RS_E_ARG:
            raise ErrInvalidInput()
        if rc != N.RS_OK:
            raise _wrapped(rc, "decode_session feed")

    def peek(self, idx: int, length: Optional[int] = None) -> bytearray:
        """The first `length` (default S) bytes of the row of a wanted or compared shard, after
        the feeds so far."""
        out = bytearray(self.S if length is None else int(length))
        one = bytearray(1)  # a zero-length peek still waits for the feeds
        rc = N.lib.rs_session_peek(self.handle, int(idx), ctypes.c_void_p(_addr(out or one)), len(out))
        if rc == N.RS_E_ARG:
            raise ErrInvalidInput()
        if rc != N.RS_OK:
            raise _wrapped(rc, "decode_session peek")
        return out

    def finish(self, dst: Optional[Sequence] = None, dst_lens: Optional[Sequence[int]] = None,
               fix: Optional[Sequence] = None) -> List[int]:
        """Closes the decode. dst: k+m entries, a writable buffer per wanted shard (None: the
        session allocates them); dst_lens: how many bytes each receives (default S). The wanted
        shards are then in self.shards. fix (repair=True): k+m entries, writable S-byte buffers
        at expected or fed compared indices into which the shards' error values are XORed.
        Returns the k+m+1 counts (zeros without repair; also kept in self.counts). Raises ErrTooFewShards before the k-th
        expected shard -- the session stays usable -- and ErrShardCorrupted, after the wanted
        shards have been written, when the compared shards do not lie on the expected shards'
        codeword (repair=True: when a column stays unexplained)."""
        n = self.k + self.m
        if dst is None:
            dst = [bytearray(self.S) if w else None for w in self.want]
        if len(dst) != n or (fix is not None and len(fix) != n) or (dst_lens is not None and len(dst_lens) != n):
            raise ErrTooFewShards()
        if any(d is not None and not _writable(d) for d in list(dst) + list(fix or [])):
            raise ErrInvalidInput()
        lens = None if dst_lens is None else (ctypes.c_size_t * n)(*[int(x) for x in dst_lens])
        counts = (ctypes.c_uint64 * (n + 1))()
        rc = N.lib.rs_session_finish(self.handle, _shard_ptrs(list(dst)), lens,
                                     None if fix is None else _shard_ptrs(list(fix)), counts)
        self.counts = list(counts)
        if rc in (N.RS_OK, N.RS_E_CORRUPT):
            self.shards = list(dst)
        if rc == N.RS_E_ARG:
            raise ErrInvalidInput()
        if rc == N.RS_E_CORRUPT:
            raise ErrShardCorrupted()
        if rc == N.RS_E_TOO_FEW_SHARDS:
            raise ErrTooFewShards()
        if rc != N.RS_OK:
            raise _wrapped(rc, "decode_session finish")
        return list(counts)

    def close(self) -> None:
        if getattr(self, "handle", None):
            N.lib.rs_session_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ObjectDecodeSession:
    """Codec.decode_session's session: a DecodeSession whose result is the joined, trimmed object.
    A delivered data shard is kept where it belongs in the object as it is fed; finish() points
    the session's destinations at the gaps, the data shards that were not fetched."""

    def __init__(self, session: DecodeSession, original_size: int):
        self.session = session
        self.size = int(original_size)
        self.out = bytearray(self.size)
        self._fed: List[int] = []

    def _span(self, i: int):
        S = self.session.S
        return min(i * S, self.size), min((i + 1) * S, self.size)

    def feed(self, idx: int, shard) -> None:
        self.session.feed(idx, shard)
        if idx < self.session.k:
            a, b = self._span(idx)
            self.out[a:b] = memoryview(shard).cast("B")[:b - a]
            self._fed.append(idx)

    def peek(self, idx: int, length: Optional[int] = None) -> bytearray:
        return self.session.peek(idx, length)

    def finish(self) -> bytearray:
        """The object's original_size bytes. Errors as DecodeSession.finish; with repair=True a
        delivered data shard the compared shards prove corrupt is restored in the object too."""
        s = self.session
        n, view = s.k + s.m, memoryview(self.out)
        dst: List = [None] * n
        lens = [0] * n
        for i in range(n):
            if s.want[i]:
                a, b = self._span(i)
                lens[i] = b - a
                dst[i] = view[a:b] if b > a else None
        fix = None
        if s.repair:
            fix = [bytearray(s.S) if i in self._fed else None for i in range(n)]
        self.counts = s.finish(dst, lens, fix)
        for i in self._fed if s.repair else ():
            if self.counts[i]:
                a, b = self._span(i)
                np.frombuffer(view[a:b], dtype=np.uint8)[:] ^= np.frombuffer(fix[i], dtype=np.uint8)[:b - a]
        return self.out

    def close(self) -> None:
        self.session.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class EncodeSession:
    """rs_encode_session_open: a progressive encode of one object of `size` bytes
    whose m parity rows stay on the device. feed(off, data) folds body bytes [off, off + len(data))
    in, from any thread and in any order, every byte exactly once; peek() reads a row's partial
    result; finish() returns the m parity shards once [0, size) is covered. A context manager:
    leaving it closes the session."""

    def __init__(self, k: int, m: int, size: int, context: Optional[N.Context] = None):
        self.ctx = context or N.default_context()
        self.k, self.m, self.size = k, m, int(size)
        self.S = (self.size + k - 1) // k if k >= 1 else 0
        self.handle = None
        h = ctypes.c_void_p()
        rc = N.lib.rs_encode_session_open(self.ctx.handle, k, m, max(self.size, 0), ctypes.byref(h))
        if rc == N.RS_E_ARG:
            raise ErrInvalidInput()
        if rc == N.RS_E_INVALID_PROFILE:
            raise ErrInvalidProfile()
        if rc != N.RS_OK:
            raise _wrapped(rc, "encode_session")
        self.handle = h

    def feed(self, off: int, data) -> None:
        """Folds body bytes [off, off + len(data)) in. Returns when `data` may be reused. A range
        that is empty, reaches past the object, overlaps anything fed before or comes after a
        finish raises ErrInvalidInput, and nothing is launched for it."""
        view = memoryview(data).cast("B")
        if off < 0 or len(view) == 0:
            raise ErrInvalidInput()
        rc = N.lib.rs_encode_session_feed(self.handle, int(off), ctypes.c_void_p(_addr(view)), len(view))
        if rc == N.RS_E_ARG:
            raise ErrInvalidInput()
        if rc != N.RS_OK:
            raise _wrapped(rc, "encode_session feed")

    def peek(self, j: int, length: Optional[int] = None) -> bytearray:
        """The first `length` (default S) bytes of parity row j, after the feeds so far."""
        out = bytearray(self.S if length is None else int(length))
        one = bytearray(1)  # a zero-length peek still waits for the feeds
        rc = N.lib.rs_encode_session_peek(self.handle, int(j), ctypes.c_void_p(_addr(out or one)), len(out))
        if rc == N.RS_E_ARG:
            raise ErrInvalidInput()
        if rc != N.RS_OK:
            raise _wrapped(rc, "encode_session peek")
        return out

    def finish(self, parity: Optional[Sequence] = None) -> List:
        """The m parity shards, S bytes each, into `parity` (m writable buffers; None: the session
        allocates them). Raises ErrShortData while [0, size) is not covered -- the session stays
        usable. May be repeated."""
        if parity is None:
            parity = [bytearray(self.S) for _ in range(self.m)]
        if len(parity) != self.m or any(p is None or not _writable(p) or len(p) < self.S for p in parity):
            raise ErrInvalidInput()
        ss = ctypes.c_size_t(0)
        rc = N.lib.rs_encode_session_finish(self.handle, _shard_ptrs(list(parity)), ctypes.byref(ss))
        if rc == N.RS_E_ARG:
            raise ErrInvalidInput()
        if rc != N.RS_OK:
            raise _wrapped(rc, "encode_session finish")
        assert ss.value == self.S
        return list(parity)

    def close(self) -> None:
        if getattr(self, "handle", None):
            N.lib.rs_encode_session_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ObjectEncodeSession:
    """Codec.encode_session's session: an EncodeSession that also keeps the fed bytes, in one
    buffer of k * S zero-initialised bytes, so that finish() can return the k + m shards as
    Codec.encode does. write(data) feeds at the running offset."""

    def __init__(self, session: EncodeSession):
        self.session = session
        self.body = bytearray(session.k * session.S)
        self.offset = 0

    def feed(self, off: int, data) -> None:
        view = memoryview(data).cast("B")
        self.session.feed(off, view)
        self.body[off:off + len(view)] = view

    def write(self, data) -> int:
        """Feeds `data` at the running offset, as an io.Writer takes a request body."""
        n = len(memoryview(data).cast("B"))
        self.feed(self.offset, data)
        self.offset += n
        return n

    def peek(self, j: int, length: Optional[int] = None) -> bytearray:
        return self.session.peek(j, length)

    def finish(self) -> List[memoryview]:
        """data_shards + parity_shards shards of S bytes, bit for bit Codec.encode's for the
        body. Errors as EncodeSession.finish."""
        s = self.session
        parity = bytearray(s.S * s.m)
        bv, pv = memoryview(self.body), memoryview(parity)
        s.finish([pv[j * s.S:(j + 1) * s.S] for j in range(s.m)])
        return [bv[i * s.S:(i + 1) * s.S] for i in range(s.k)] + [pv[j * s.S:(j + 1) * s.S] for j in range(s.m)]

    def close(self) -> None:
        self.session.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def verify(shards: List, k: int, m: int, context: Optional[N.Context] = None) -> bool:
    """upstream enc.Verify(shards) (codec.go:59)."""
    ctx = context or N.default_context()
    n = k + m
    if len(shards) != n:
        raise ErrTooFewShards()
    lens = (ctypes.c_size_t * n)(*[0 if s is None else len(s) for s in shards])
    ok = ctypes.c_int(0)
    rc = N.lib.rs_verify(ctx.handle, k, m, _shard_ptrs(shards), lens, ctypes.byref(ok))
    if rc != N.RS_OK:
        raise _wrapped(rc, "verify")
    return bool(ok.value)


# ---- batched host calls (many independent stripes per native call) ----------------

def encode_batch(stripes: Sequence[Sequence], k: int, m: int,
                 context: Optional[N.Context] = None) -> Tuple[List[List[bytearray]], List[int]]:
    """rs_encode_batch: stripes[b] holds the k data shards of stripe b (equal length
    within a stripe; stripes may differ). Returns (parity[b] = m fresh shards, status[b])
    with status[b] one of RS_OK / RS_E_NO_DATA (empty shards)."""
    ctx = context or N.default_context()
    B = len(stripes)
    sizes = (ctypes.c_size_t * max(B, 1))()
    parity = []
    for b, st in enumerate(stripes):
        if len(st) != k:
            raise ErrTooFewShards()
        S = len(st[0])
        if any(len(s) != S for s in st):
            raise ErrShardSize()
        sizes[b] = S
        parity.append([bytearray(S) for _ in range(m)])
    data = _shard_ptrs([s for st in stripes for s in st] or [None])
    par = _shard_ptrs([p for ps in parity for p in ps] or [None])
    status = (ctypes.c_int * max(B, 1))()
    rc = N.lib.rs_encode_batch(ctx.handle, k, m, B, sizes, data, par, status)
    if rc not in (N.RS_OK, N.RS_E_NO_DATA):
        N.check(rc, "rs_encode_batch")
    return parity, list(status)[:B]


def reconstruct_batch(stripes: List[List], k: int, m: int, verify: bool = True,
                      context: Optional[N.Context] = None, required=None) -> List[int]:
    """rs_reconstruct_batch: stripes[b] is an n-list of shards (None / empty = missing),
    reconstructed in place like reconstruct(); with verify the present parity beyond the
    first k is re-checked per stripe. Returns status[b] (RS_OK, RS_E_CORRUPT,
    RS_E_TOO_FEW_SHARDS, RS_E_SHARD_SIZE, RS_E_NO_DATA, ...).
    required: None, or per stripe k+m flags (rs_reconstruct_some_batch): only the missing
    entries whose flag is set are rebuilt and replaced."""
    ctx = context or N.default_context()
    n = k + m
    B = len(stripes)
    if any(len(st) != n for st in stripes):
        raise ErrTooFewShards()
    if required is not None and (len(required) != B or any(len(r) != n for r in required)):
        raise ValueError("required: None, or one row of k+m flags per stripe")
    # missing entries get fresh buffers in a per-stripe copy (upstream Reconstruct
    # allocates them); the caller's lists change only for stripes that succeeded
    flat, lens, bufs = [], (ctypes.c_size_t * max(B * n, 1))(), []
    for b, st in enumerate(stripes):
        ln = [0 if s is None else len(s) for s in st]
        S = next((x for x in ln if x), 0)
        cp = list(st)
        for i in range(n):
            lens[b * n + i] = ln[i]
            if ln[i] == 0 and S and (required is None or required[b][i]):
                cp[i] = bytearray(S)
        bufs.append(cp)
        flat += cp
    status = (ctypes.c_int * max(B, 1))()
    if required is None:
        rc = N.lib.rs_reconstruct_batch(ctx.handle, k, m, B, _shard_ptrs(flat or [None]), lens,
                                        int(verify), status)
    else:
        req = (ctypes.c_uint8 * max(B * n, 1))(*[1 if f else 0 for r in required for f in r])
        rc = N.lib.rs_reconstruct_some_batch(ctx.handle, k, m, B, _shard_ptrs(flat or [None]), lens,
                                             req, int(verify), status)
    if rc < 0 and rc not in (N.RS_E_CORRUPT, N.RS_E_TOO_FEW_SHARDS, N.RS_E_SHARD_SIZE,
                             N.RS_E_NO_DATA):
        if not (rc == N.RS_E_ARG and any(s == N.RS_E_ARG for s in list(status)[:B])):
            N.check(rc, "rs_reconstruct_batch")
    out = list(status)[:B]
    for b, st in enumerate(stripes):
        if out[b] in (N.RS_OK, N.RS_E_CORRUPT):
            for i in range(n):
                if (st[i] is None or len(st[i]) == 0) and lens[b * n + i]:
                    st[i] = bufs[b][i]
    return out


def _per_stripe(rc: int, status: Sequence[int], what: str) -> None:
    """Raises for a call-level error of a batch call: a code no stripe reports."""
    if rc < 0 and rc not in status:
        N.check(rc, what)


def locate(shards: List, k: int, m: int, context: Optional[N.Context] = None,
           max_errors: int = 1) -> np.ndarray:
    """rs_locate: which shard of a stripe is corrupt. shards: an n-list
    (None / empty = missing); nothing is written. Returns k+m+1 uint64 counts: [i] = byte
    columns blamed on shard i, [k+m] = columns that mismatch but that no single shard
    explains. All zero for a clean stripe (and for one with exactly k shards present).
    max_errors=2 (rs_locate_ex, §5.12.1): a column in which two shards are corrupt counts once
    for each of the two, where the stripe compares four or more shards."""
    _check_max_errors(max_errors, "rs_locate_ex")
    ctx = context or N.default_context()
    n = k + m
    if len(shards) != n:
        raise ErrTooFewShards()
    lens = (ctypes.c_size_t * n)(*[0 if s is None else len(s) for s in shards])
    counts = np.zeros(n + 1, dtype=np.uint64)
    rc = N.lib.rs_locate_ex(ctx.handle, k, m, _shard_ptrs(shards), lens,
                            counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), int(max_errors))
    if rc not in (N.RS_OK, N.RS_E_CORRUPT):
        raise _wrapped(rc, "locate")
    return counts


def locate_batch(stripes: Sequence[Sequence], k: int, m: int,
                 context: Optional[N.Context] = None,
                 max_errors: int = 1) -> Tuple[np.ndarray, List[int]]:
    """rs_locate_batch: locate() for many stripes of any sizes and erasures in one call.
    Returns (counts, a (batch, k+m+1) uint64 array; status[b]: RS_OK, RS_E_CORRUPT where a
    column mismatched, or the stripe's own error as reconstruct_batch reports it).
    max_errors as for locate() (rs_locate_batch_ex)."""
    _check_max_errors(max_errors, "rs_locate_batch_ex")
    ctx = context or N.default_context()
    n = k + m
    B = len(stripes)
    if any(len(st) != n for st in stripes):
        raise ErrTooFewShards()
    lens = (ctypes.c_size_t * max(B * n, 1))(*[0 if s is None else len(s) for st in stripes for s in st])
    counts = np.zeros((B, n + 1), dtype=np.uint64)
    status = (ctypes.c_int * max(B, 1))()
    rc = N.lib.rs_locate_batch_ex(ctx.handle, k, m, B, _shard_ptrs([s for st in stripes for s in st] or [None]),
                                  lens, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), status,
                                  int(max_errors))
    out = list(status)[:B]
    _per_stripe(rc, out, "rs_locate_batch")
    return counts, out


def heal_batch(stripes: List[List], k: int, m: int,
               context: Optional[N.Context] = None,
               max_errors: int = 1) -> Tuple[List[int], List[List[int]]]:
    """rs_heal_batch: reconstruct_batch(verify=True) that repairs what it can. A stripe whose
    compared shards mismatch is located; when the blamed shards explain every mismatching
    column and a compared shard is left to confirm with, they are rebuilt in place (writable
    buffers) together with the missing ones and the stripe verified again. Returns
    (status[b], healed[b] = indices of the shards rebuilt because they were corrupt).
    max_errors=2 (rs_heal_batch_ex, §5.12.1) also heals shards that are corrupt in the same
    byte columns, two per column, where four or more shards are compared."""
    _check_max_errors(max_errors, "rs_heal_batch_ex")
    ctx = context or N.default_context()
    n = k + m
    B = len(stripes)
    if any(len(st) != n for st in stripes):
        raise ErrTooFewShards()
    flat, lens, bufs = [], (ctypes.c_size_t * max(B * n, 1))(), []
    for b, st in enumerate(stripes):
        ln = [0 if s is None else len(s) for s in st]
        S = next((x for x in ln if x), 0)
        cp = list(st)
        for i in range(n):
            lens[b * n + i] = ln[i]
            if ln[i] == 0 and S:
                cp[i] = bytearray(S)
            elif ln[i] and not _writable(cp[i]):
                raise TypeError("heal_batch rebuilds corrupt shards in place: writable buffers")
        bufs.append(cp)
        flat += cp
    status = (ctypes.c_int * max(B, 1))()
    healed = (ctypes.c_uint8 * max(B * n, 1))()
    rc = N.lib.rs_heal_batch_ex(ctx.handle, k, m, B, _shard_ptrs(flat or [None]), lens, healed, status,
                                int(max_errors))
    out = list(status)[:B]
    _per_stripe(rc, out, "rs_heal_batch")
    for b, st in enumerate(stripes):
        if out[b] in (N.RS_OK, N.RS_E_CORRUPT):
            for i in range(n):
                if (st[i] is None or len(st[i]) == 0) and lens[b * n + i]:
                    st[i] = bufs[b][i]
    return out, [[i for i in range(n) if healed[b * n + i]] for b in range(B)]


def _need_writable(stripes: Sequence[Sequence], call: str) -> None:
    for st in stripes:
        for s in st:
            if s is not None and len(s) and not _writable(s):
                raise TypeError(f"{call} repairs corrupt bytes in place: writable buffers")


def correct(shards: List, k: int, m: int, context: Optional[N.Context] = None) -> np.ndarray:
    """rs_correct: repairs, in place, every byte column of a stripe in which
    one examined shard is corrupt, where the stripe compares three or more shards. shards: an
    n-list of writable buffers (None / empty = missing: neither read nor rebuilt). Returns
    k+m+1 uint64 counts: [i] = bytes of shard i that were changed, [k+m] = columns that still
    mismatch (more than one error, or fewer than three compared shards)."""
    ctx = context or N.default_context()
    n = k + m
    if len(shards) != n:
        raise ErrTooFewShards()
    _need_writable([shards], "correct")
    lens = (ctypes.c_size_t * n)(*[0 if s is None else len(s) for s in shards])
    counts = np.zeros(n + 1, dtype=np.uint64)
    rc = N.lib.rs_correct(ctx.handle, k, m, _shard_ptrs(shards), lens,
                          counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    if rc not in (N.RS_OK, N.RS_E_CORRUPT):
        raise _wrapped(rc, "correct")
    return counts


def correct_batch(stripes: Sequence[Sequence], k: int, m: int,
                  context: Optional[N.Context] = None) -> Tuple[np.ndarray, List[int]]:
    """rs_correct_batch: correct() for many stripes of any sizes and erasures in one call.
    Returns (counts, a (batch, k+m+1) uint64 array; status[b]: RS_OK where nothing mismatched
    or every mismatching column was corrected, RS_E_CORRUPT where a column is left, or the
    stripe's own error as reconstruct_batch reports it). Only shards with corrected bytes are
    copied back from the device."""
    ctx = context or N.default_context()
    n = k + m
    B = len(stripes)
    if any(len(st) != n for st in stripes):
        raise ErrTooFewShards()
    _need_writable(stripes, "correct_batch")
    lens = (ctypes.c_size_t * max(B * n, 1))(*[0 if s is None else len(s) for st in stripes for s in st])
    counts = np.zeros((B, n + 1), dtype=np.uint64)
    status = (ctypes.c_int * max(B, 1))()
    rc = N.lib.rs_correct_batch(ctx.handle, k, m, B, _shard_ptrs([s for st in stripes for s in st] or [None]),
                                lens, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), status)
    out = list(status)[:B]
    _per_stripe(rc, out, "rs_correct_batch")
    return counts, out


def host_counters(context: Optional[N.Context] = None) -> dict:
    """rs_host_counters_read: the context's monotonic counts of host-memory calls that
    reached a device (`calls`), chunks sent (`chunks`), compute launches (`launches`, one per
    launch group per chunk), H2D / D2H / memset dispatches (`copies`) and batch calls that took
    the ragged path (`ragged_calls`)."""
    ctx = context or N.default_context()
    c = N.HostCounters()
    N.check(N.lib.rs_host_counters_read(ctx.handle, ctypes.byref(c)), "rs_host_counters_read")
    return {name: int(getattr(c, name)) for name, _ in c._fields_}


# ---- host-side matrices (no device needed) ------------------------------------------

def encode_matrix(k: int, m: int) -> np.ndarray:
    """(k+m) x k systematic matrix E = V . inv(V[0:k]) (upstream buildMatrix)."""
    E = np.zeros((k + m, k), dtype=np.uint8)
    rc = N.lib.rs_encode_matrix(k, m, E.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    if rc == N.RS_E_INVALID_PROFILE:
        raise ErrInvalidProfile()
    N.check(rc, "rs_encode_matrix")
    return E


def decode_rows(k: int, m: int, present: Sequence[bool]):
    """(valid, missing, rows) as the fused decode kernel applies them."""
    n = k + m
    pr = np.array([1 if p else 0 for p in present], dtype=np.uint8)
    valid = (ctypes.c_int * k)()
    missing = (ctypes.c_int * n)()
    nm = ctypes.c_int(0)
    rows = np.zeros((n, k), dtype=np.uint8)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    rc = N.lib.rs_decode_rows(k, m, pr.ctypes.data_as(u8), valid, missing, ctypes.byref(nm),
                              rows.ctypes.data_as(u8))
    if rc != N.RS_OK:
        raise _wrapped(rc, "decode_rows")
    return list(valid), list(missing)[:nm.value], rows[:nm.value]
