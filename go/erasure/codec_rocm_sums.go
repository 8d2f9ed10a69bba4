//go:build rocm && cgo

// Checksummed batches (DESIGN.md §7.7): EncodeBatch that also returns every shard's
// ShardChecksum, and DecodeBatch that checks every present shard against its recorded
// checksum, drops a mismatching shard and heals it -- what Manager.StoreFile
// (manager.go:185) and Manager.RetrieveFile (manager.go:283-296) do around the codec, taken
// on the way through the pipeline instead of in a second pass over the shards on the CPU.
// Not in the reference API: additions for a server that batches small uploads and downloads.
package erasure

/*
#include <stdlib.h>
#include "callfs_rs.h"
*/
import "C"

import (
	"encoding/hex"
	"fmt"
	"runtime"
	"unsafe"

	"github.com/klauspost/reedsolomon"
)

// EncodeBatchSums is EncodeBatch plus sums[b][i] = ShardChecksum(out[b][i]) for every object
// that encoded (rs_codec_encode_batch_sums); sums[b] is nil where errs[b] is set.
func (c *Codec) EncodeBatchSums(objs [][]byte, profile ErasureProfile) ([][][]byte, [][]string, []error) {
	k, m := profile.DataShards, profile.ParityShards
	out := make([][][]byte, len(objs))
	sums := make([][]string, len(objs))
	errs := make([]error, len(objs))
	if k < 1 || m < 1 {
		for b := range errs {
			errs[b] = ErrInvalidProfile
		}
		return out, sums, errs
	}
	if len(objs) == 0 {
		return out, sums, errs
	}
	n := k + m
	if n > 256 || device() == nil {
		return cpuEncodeBatchSums(c, objs, profile)
	}
	B := len(objs)
	data, dst := newCArray(B), newCArray(B)
	defer data.free()
	defer dst.free()
	lens := make([]C.size_t, B) // Go memory without Go pointers: may be passed
	caps := make([]C.size_t, B)
	sizes := make([]C.size_t, B)
	status := make([]C.int, B)
	digests := make([]byte, B*n*32)
	bufs := make([][]byte, B)
	var pin runtime.Pinner
	defer pin.Unpin()
	for b, d := range objs {
		lens[b] = C.size_t(len(d))
		if len(d) == 0 {
			continue // reports RS_E_SHORT_DATA, as upstream Split does
		}
		S := (len(d) + k - 1) / k
		if cap(d) >= n*S {
			bufs[b] = d[:n*S] // in place: the pad and the parity land in the spare capacity
		} else {
			bufs[b] = make([]byte, n*S)
		}
		caps[b] = C.size_t(n * S)
		pin.Pin(&d[0])
		pin.Pin(&bufs[b][0])
		data.set(b, unsafe.Pointer(&d[0]))
		dst.set(b, unsafe.Pointer(&bufs[b][0]))
	}
	rc := C.rs_codec_encode_batch_sums(gpuCtx, C.int(k), C.int(m), C.int(B), data.at(0), &lens[0],
		dst.at(0), &caps[0], &sizes[0], (*C.uint8_t)(unsafe.Pointer(&digests[0])), &status[0])
	if rc != C.RS_OK && !hasStatus(status, rc) { // a call-level error: no status was written
		for b := range errs {
			errs[b] = fmt.Errorf("erasure: failed to encode parity: %w", upstreamErr(rc))
		}
		return out, sums, errs
	}
	for b := range objs {
		switch st := status[b]; st {
		case C.RS_OK:
			S := int(sizes[b])
			out[b] = make([][]byte, n)
			sums[b] = make([]string, n)
			for i := range out[b] {
				out[b][i] = bufs[b][i*S : (i+1)*S : (i+1)*S]
				sums[b][i] = hex.EncodeToString(digests[(b*n+i)*32 : (b*n+i+1)*32])
			}
		case C.RS_E_SHORT_DATA:
			errs[b] = fmt.Errorf("erasure: failed to split data: %w", upstreamErr(st))
		default:
			errs[b] = fmt.Errorf("erasure: failed to encode parity: %w", upstreamErr(st))
		}
	}
	return out, sums, errs
}

// DecodeBatchSums is DecodeBatch with the retrieve side's checksum pass folded in
// (rs_codec_decode_batch_sums). sums[b][i] is the recorded ShardChecksum of shard i of object
// b (entries of missing shards are ignored). A present shard that does not match is treated as
// missing, as manager.go:283-296 treats it: bad[b] lists those shards, each is rebuilt into
// its own slice, and errs[b] is what Decode reports for the object without them
// (ErrTooFewShards where fewer than k good shards are left; the object's shards are then left
// as given). One difference from the manager: a present shard of the wrong length is a shard
// size error here, where the manager would see a checksum mismatch -- drop such a shard
// (ShardSize is in the metadata) before the call.
func (c *Codec) DecodeBatchSums(shards [][][]byte, sums [][]string, profile ErasureProfile, sizes []int64) ([][]byte, [][]int, []error) {
	k, m := profile.DataShards, profile.ParityShards
	out := make([][]byte, len(shards))
	bad := make([][]int, len(shards))
	errs := make([]error, len(shards))
	if k < 1 || m < 1 || len(sizes) != len(shards) || len(sums) != len(shards) {
		for b := range errs {
			errs[b] = ErrInvalidProfile
			if k >= 1 && m >= 1 {
				errs[b] = fmt.Errorf("erasure: %d sizes and %d checksum lists for %d objects", len(sizes), len(sums), len(shards))
			}
		}
		return out, bad, errs
	}
	if len(shards) == 0 {
		return out, bad, errs
	}
	n := k + m
	if n > 256 || device() == nil {
		return cpuDecodeBatchSums(c, shards, sums, profile, sizes)
	}
	B := len(shards)
	bufs := make([][][]byte, B)
	ptrs, outs := newCArray(B*n), newCArray(B)
	defer ptrs.free()
	defer outs.free()
	lens := make([]C.size_t, B*n) // Go memory without Go pointers: may be passed
	osz := make([]C.int64_t, B)
	status := make([]C.int, B)
	expected := make([]byte, B*n*32)
	flags := make([]byte, B*n)
	var pin runtime.Pinner
	defer pin.Unpin()
	for b, sh := range shards {
		if len(sh) != n || len(sums[b]) != n {
			errs[b] = fmt.Errorf("erasure: reconstruction failed: %w", reedsolomon.ErrTooFewShards)
			continue // all lens 0 and no pointers: the object reports RS_E_NO_DATA, ignored
		}
		S := 0
		for _, s := range sh {
			if len(s) > 0 {
				S = len(s)
				break
			}
		}
		bufs[b] = make([][]byte, n)
		copy(bufs[b], sh)
		for i, s := range bufs[b] {
			lens[b*n+i] = C.size_t(len(s))
			if len(s) == 0 && S > 0 {
				if cap(s) >= S {
					s = s[:S]
				} else {
					s = make([]byte, S)
				}
				bufs[b][i] = s
			} else if len(s) > 0 {
				// a checksum that is no 64-digit hex string matches no shard: zeros stay
				if d, err := hex.DecodeString(sums[b][i]); err == nil && len(d) == 32 {
					copy(expected[(b*n+i)*32:], d)
				}
			}
			if len(s) > 0 {
				pin.Pin(&s[0])
				ptrs.set(b*n+i, unsafe.Pointer(&s[0]))
			}
		}
		osz[b] = C.int64_t(sizes[b])
		if sizes[b] > 0 {
			out[b] = make([]byte, sizes[b])
			pin.Pin(&out[b][0])
			outs.set(b, unsafe.Pointer(&out[b][0]))
		}
	}
	rc := C.rs_codec_decode_batch_sums(gpuCtx, C.int(k), C.int(m), C.int(B), ptrs.at(0), &lens[0],
		(*C.uint8_t)(unsafe.Pointer(&expected[0])), outs.at(0), &osz[0],
		(*C.uint8_t)(unsafe.Pointer(&flags[0])), &status[0])
	callLevel := rc != C.RS_OK && !hasStatus(status, rc) // no status was written
	for b, sh := range shards {
		if errs[b] != nil {
			out[b] = nil
			continue
		}
		st := status[b]
		if callLevel {
			st = rc
		}
		for i := 0; !callLevel && i < n; i++ {
			if flags[b*n+i] != 0 {
				bad[b] = append(bad[b], i)
			}
		}
		switch st {
		case C.RS_OK, C.RS_E_CORRUPT, C.RS_E_INSUFFICIENT:
			// Reconstruct ran: upstream has filled the nil entries by now (codec.go:55); a bad
			// shard was rebuilt inside its own slice
			for i := range sh {
				if len(sh[i]) == 0 && lens[b*n+i] != 0 {
					sh[i] = bufs[b][i]
				}
			}
		}
		if st != C.RS_OK {
			out[b] = nil
		} else if out[b] == nil {
			out[b] = []byte{} // an empty object, as Decode's buf[:0]
		}
		errs[b] = decodeErr(st)
	}
	return out, bad, errs
}
