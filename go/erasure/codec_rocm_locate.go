//go:build rocm && cgo

// Locate and heal (DESIGN.md §5.12): which shard of an object is corrupt, from the parity
// syndromes alone, and a Decode that repairs what they name. Not in the reference API: the
// reference finds a bad shard by hashing every shard against the metadata
// (manager.go:250-320); these calls need no checksum and cost one more pass over the shards.
// The ...Max variants (§5.12.1) take the number of corrupt shards a byte column may be blamed
// on: 1 is the plain call, 2 also names two shards that are corrupt in the same columns where
// four or more shards are compared.
package erasure

/*
#include <stdlib.h>
#include "callfs_rs.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"unsafe"

	"github.com/klauspost/reedsolomon"
)

// ErrLocateUnavailable is what Locate reports where no device can run it (a build without
// the GPU codec, no usable device, k+m > 256): the CPU codec has no locator.
var ErrLocateUnavailable = errors.New("erasure: locating corrupt shards needs the GPU codec")

// pinShards fills ptrs / lens for one object's n shards (nil or empty = missing).
func pinShards(pin *runtime.Pinner, ptrs cArray, lens []C.size_t, at int, shards [][]byte) {
	for i, s := range shards {
		lens[at+i] = C.size_t(len(s))
		if len(s) > 0 {
			pin.Pin(&s[0])
			ptrs.set(at+i, unsafe.Pointer(&s[0]))
		}
	}
}

// Locate reports, per shard of one object, in how many byte columns that shard alone is
// corrupt (rs_locate): counts[i] for shard i, and counts[k+m] for the columns that mismatch
// but that no single shard explains. Nothing is written. An object with exactly k shards
// present has nothing to compare and reports zeros. A scrub calls it (or HealBatch) per
// object instead of hashing every shard.
func (c *Codec) Locate(shards [][]byte, profile ErasureProfile) ([]uint64, error) {
	return c.LocateMax(shards, profile, 1)
}

// ErrMaxErrors is what the ...Max calls report for maxErrors outside 1..2.
var ErrMaxErrors = errors.New("erasure: maxErrors must be 1 or 2")

// LocateMax is Locate with maxErrors corrupt shards per byte column (rs_locate_ex). With 2, a
// column in which two shards are corrupt counts once for each of the two, so the counts may add
// up to more than the shard size.
func (c *Codec) LocateMax(shards [][]byte, profile ErasureProfile, maxErrors int) ([]uint64, error) {
	if maxErrors < 1 || maxErrors > 2 {
		return nil, ErrMaxErrors
	}
	k, m := profile.DataShards, profile.ParityShards
	if k < 1 || m < 1 {
		return nil, ErrInvalidProfile
	}
	n := k + m
	if n > 256 || device() == nil {
		return nil, ErrLocateUnavailable
	}
	if len(shards) != n {
		return nil, fmt.Errorf("erasure: reconstruction failed: %w", reedsolomon.ErrTooFewShards)
	}
	ptrs := newCArray(n)
	defer ptrs.free()
	lens := make([]C.size_t, n)
	counts := make([]C.uint64_t, n+1)
	var pin runtime.Pinner
	defer pin.Unpin()
	pinShards(&pin, ptrs, lens, 0, shards)
	rc := C.rs_locate_ex(gpuCtx, C.int(k), C.int(m), ptrs.at(0), &lens[0], &counts[0], C.int(maxErrors))
	if rc != C.RS_OK && rc != C.RS_E_CORRUPT { // RS_E_CORRUPT: the counts say where
		return nil, decodeErr(rc)
	}
	out := make([]uint64, n+1)
	for i := range out {
		out[i] = uint64(counts[i])
	}
	return out, nil
}

// HealBatch is RepairBatch that repairs corrupt shards too (rs_heal_batch). An object whose
// present shards beyond the first k mismatch is located; when the blamed shards explain every
// mismatching column and a compared shard is left to confirm with, they are rebuilt in place
// together with the missing ones and the object verified again. errs[b] is what RepairBatch
// reports, with ErrShardCorrupted left for the objects beyond repair; healed[b] lists the
// shard indices of object b that were corrupt and have been rewritten (the caller stores them
// back). Present shards that nobody blamed are never written.
func (c *Codec) HealBatch(objs [][][]byte, profile ErasureProfile) (healed [][]int, errs []error) {
	return c.HealBatchMax(objs, profile, 1)
}

// HealBatchMax is HealBatch with maxErrors corrupt shards per byte column (rs_heal_batch_ex):
// with 2 it also heals shards that are corrupt in the same columns, two per column, as long as
// a compared shard is left to confirm with.
func (c *Codec) HealBatchMax(objs [][][]byte, profile ErasureProfile, maxErrors int) (healed [][]int, errs []error) {
	k, m := profile.DataShards, profile.ParityShards
	errs = make([]error, len(objs))
	healed = make([][]int, len(objs))
	if maxErrors < 1 || maxErrors > 2 {
		for b := range errs {
			errs[b] = ErrMaxErrors
		}
		return healed, errs
	}
	if k < 1 || m < 1 {
		for b := range errs {
			errs[b] = ErrInvalidProfile
		}
		return healed, errs
	}
	n := k + m
	if len(objs) == 0 {
		return healed, errs
	}
	if n > 256 || device() == nil {
		return healed, c.RepairBatch(objs, profile)
	}
	bufs := make([][][]byte, len(objs))
	ptrs := newCArray(len(objs) * n)
	defer ptrs.free()
	lens := make([]C.size_t, len(objs)*n)
	flags := make([]C.uint8_t, len(objs)*n)
	status := make([]C.int, len(objs))
	var pin runtime.Pinner
	defer pin.Unpin()
	for b, shards := range objs {
		if len(shards) != n {
			errs[b] = fmt.Errorf("erasure: reconstruction failed: %w", reedsolomon.ErrTooFewShards)
			continue // all lens 0 and no pointers: the stripe reports RS_E_NO_DATA, ignored
		}
		S := 0
		for _, s := range shards {
			if len(s) > 0 {
				S = len(s)
				break
			}
		}
		bufs[b] = make([][]byte, n)
		copy(bufs[b], shards)
		for i, s := range bufs[b] {
			lens[b*n+i] = C.size_t(len(s))
			if len(s) == 0 && S > 0 {
				s = make([]byte, S)
				bufs[b][i] = s
			}
			if len(s) > 0 {
				pin.Pin(&s[0])
				ptrs.set(b*n+i, unsafe.Pointer(&s[0]))
			}
		}
	}
	rc := C.rs_heal_batch_ex(gpuCtx, C.int(k), C.int(m), C.int(len(objs)), ptrs.at(0), &lens[0],
		&flags[0], &status[0], C.int(maxErrors))
	if rc != C.RS_OK && !hasStatus(status, rc) { // a call-level error
		for b := range errs {
			if errs[b] == nil {
				errs[b] = decodeErr(rc)
			}
		}
		return healed, errs
	}
	for b, shards := range objs {
		if errs[b] != nil {
			continue
		}
		st := status[b]
		if st == C.RS_OK || st == C.RS_E_CORRUPT {
			for i := range shards {
				if len(shards[i]) == 0 && lens[b*n+i] != 0 {
					shards[i] = bufs[b][i]
				}
				if flags[b*n+i] != 0 {
					healed[b] = append(healed[b], i)
				}
			}
		}
		errs[b] = decodeErr(st)
	}
	return healed, errs
}

// DecodeHeal is Decode with the heal in place of the bare Verify failure
// (rs_codec_decode_heal): where Decode returns ErrShardCorrupted and the object holds enough
// redundancy to name and rebuild its corrupt shards, DecodeHeal returns the object and the
// indices of the shards it rewrote in `shards`, for the caller to store back. Every other
// error, the join and the trim are Decode's. Objects the GPU does not take (below
// CALLFS_ERASURE__GPU_MIN_BYTES, k+m > 256, no device) are decoded by the CPU codec, which
// heals nothing.
func (c *Codec) DecodeHeal(shards [][]byte, profile ErasureProfile, originalSize int64) ([]byte, []int, error) {
	return c.DecodeHealMax(shards, profile, originalSize, 1)
}

// DecodeHealMax is DecodeHeal with maxErrors corrupt shards per byte column
// (rs_codec_decode_heal_ex).
func (c *Codec) DecodeHealMax(shards [][]byte, profile ErasureProfile, originalSize int64, maxErrors int) ([]byte, []int, error) {
	if maxErrors < 1 || maxErrors > 2 {
		return nil, nil, ErrMaxErrors
	}
	k, m := profile.DataShards, profile.ParityShards
	if k < 1 || m < 1 {
		return nil, nil, ErrInvalidProfile
	}
	n := k + m
	if n > 256 || originalSize < int64(gpuMinBytes) || device() == nil {
		out, err := c.cpuDecode(shards, profile, originalSize)
		return out, nil, err
	}
	if len(shards) != n {
		return nil, nil, fmt.Errorf("erasure: reconstruction failed: %w", reedsolomon.ErrTooFewShards)
	}
	S := 0
	for _, s := range shards {
		if len(s) != 0 {
			S = len(s)
			break
		}
	}
	bufs := make([][]byte, n)
	copy(bufs, shards)
	ptrs := newCArray(n)
	defer ptrs.free()
	lens := make([]C.size_t, n)
	flags := make([]C.uint8_t, n)
	var pin runtime.Pinner
	defer pin.Unpin()
	for i := range bufs {
		if len(bufs[i]) == 0 && S > 0 {
			lens[i] = 0
			if cap(bufs[i]) >= S {
				bufs[i] = bufs[i][:S]
			} else {
				bufs[i] = make([]byte, S)
			}
			pin.Pin(&bufs[i][0])
			ptrs.set(i, unsafe.Pointer(&bufs[i][0]))
			continue
		}
		lens[i] = C.size_t(len(bufs[i]))
		if len(bufs[i]) > 0 {
			pin.Pin(&bufs[i][0])
			ptrs.set(i, unsafe.Pointer(&bufs[i][0]))
		}
	}
	buf := make([]byte, int(originalSize))
	var out *C.uint8_t
	if originalSize > 0 {
		pin.Pin(&buf[0])
		out = (*C.uint8_t)(unsafe.Pointer(&buf[0]))
	}
	rc := C.rs_codec_decode_heal_ex(gpuCtx, C.int(k), C.int(m), ptrs.at(0), &lens[0], out,
		C.int64_t(originalSize), &flags[0], C.int(maxErrors))
	switch rc {
	case C.RS_OK, C.RS_E_CORRUPT, C.RS_E_INSUFFICIENT: // Reconstruct ran: the nil entries are filled
		for i := range shards {
			if len(shards[i]) == 0 && lens[i] != 0 {
				shards[i] = bufs[i]
			}
		}
	}
	if rc != C.RS_OK {
		return nil, nil, decodeErr(rc)
	}
	var healed []int
	for i := range flags {
		if flags[i] != 0 {
			healed = append(healed, i)
		}
	}
	return buf, healed, nil
}
