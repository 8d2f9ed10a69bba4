//go:build rocm && cgo

// GPU Reed-Solomon codec for CallFS on MI355X: the cgo side of the drop-in described in
// INTEGRATION.md. It replaces the two Codec methods of erasure/codec.go (Encode at
// :21-41, Decode at :45-78) on a `-tags rocm` build; NewCodec, ShardChecksum, the
// errors (errors.go) and ErasureProfile (metadata.go) stay the reference's own.
// codec.go.diff renames the reference's methods to cpuEncode / cpuDecode, which this
// file falls back to (and codec_cpu.go calls on every other build).
//
// Build: CGO_ENABLED=1 CGO_CFLAGS=-I<repo>/include CGO_LDFLAGS="-L<lib dir>" go build -tags rocm
package erasure

/*
#cgo LDFLAGS: -lcallfs_rs
#include <stdlib.h>
#include "callfs_rs.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"os"
	"runtime"
	"strconv"
	"sync"
	"unsafe"

	"github.com/klauspost/reedsolomon"
)

var (
	gpuOnce sync.Once
	gpuCtx  *C.rs_ctx // nil: no usable device, every call takes the CPU codec
	// CALLFS_ERASURE__GPU_MIN_BYTES: objects below this stay on the CPU codec
	// (INTEGRATION.md "when the GPU pays"). 64 MiB is where one GPU call passes one CPU
	// thread on the round-6 build (DESIGN.md §7.4 "CPU or GPU", tools/jobs.sh n1_r06,
	// profiles/r06/n1/): RS(10,4) 28.2 vs 20.0 GiB/s from pageable buffers and 33.0 through
	// pinned bodies (BodyBuffer), RS(4,2) 34.7 vs 29.3 through pinned bodies; at 16 MiB the
	// cache-resident CPU port leads (51-53 vs 20-33); one threshold for every profile.
	gpuMinBytes = envInt("CALLFS_ERASURE__GPU_MIN_BYTES", 64<<20)
)

func envInt(name string, def int) int {
	if v, err := strconv.Atoi(os.Getenv(name)); err == nil && v >= 0 {
		return v
	}
	return def
}

// device returns the process-wide context, created on first use. One rs_ctx serves
// every goroutine (all rs_* calls are thread-safe), like the shared *Codec at
// manager.go:60. CALLFS_ERASURE__GPU_MASK selects devices (bit d = HIP device d).
func device() *C.rs_ctx {
	gpuOnce.Do(func() {
		mask, _ := strconv.ParseUint(os.Getenv("CALLFS_ERASURE__GPU_MASK"), 0, 32)
		var c *C.rs_ctx
		if C.rs_init(&c, C.uint(mask)) == C.RS_OK {
			gpuCtx = c
		}
	})
	return gpuCtx
}

// upstreamErr maps an rs_* code to the reedsolomon error value the CPU codec would
// have returned, so errors.Is and the wrapped .Error() text match codec.go.
func upstreamErr(rc C.int) error {
	switch rc {
	case C.RS_E_SHORT_DATA:
		return reedsolomon.ErrShortData
	case C.RS_E_TOO_FEW_SHARDS:
		return reedsolomon.ErrTooFewShards
	case C.RS_E_NO_DATA:
		return reedsolomon.ErrShardNoData
	case C.RS_E_SHARD_SIZE:
		return reedsolomon.ErrShardSize
	case C.RS_E_SINGULAR:
		return reedsolomon.ErrSingular
	}
	return errors.New(C.GoString(C.rs_strerror(rc)))
}

// decodeErr maps rs_codec_decode / rs_reconstruct_batch codes the way Decode reports
// them: the erasure package's sentinels by identity (codec.go:63-65, :73-75), anything
// from Reconstruct inside its wrapper (codec.go:56).
func decodeErr(rc C.int) error {
	switch rc {
	case C.RS_OK:
		return nil
	case C.RS_E_CORRUPT:
		return ErrShardCorrupted
	case C.RS_E_INSUFFICIENT:
		return ErrInsufficientShards
	case C.RS_E_INVALID_PROFILE:
		return ErrInvalidProfile
	}
	return fmt.Errorf("erasure: reconstruction failed: %w", upstreamErr(rc))
}

// ---- pinned host buffers (zero-copy bodies) -------------------------------------------
//
// HostBuffer / BodyBuffer hand out page-locked host memory from rs_host_alloc as Go byte
// slices (C memory: cgo's pointer rules and runtime.Pinner do not apply to it, and the GC
// never moves it). When every shard of a call lies inside such buffers, the library runs
// the call zero-copy: H2D, kernels and D2H straight on these bytes, no CPU copy through its
// staging (include/callfs_rs.h rs_host_alloc; DESIGN.md §7.4, 38-45 GiB/s for objects of
// 10 MiB and up on one request thread). Upload bodies read into a BodyBuffer instead of
// io.ReadAll's heap slice (post_file_enhanced.go:125-127) and shards fetched into
// HostBuffers instead of io.ReadAll (manager.go:473,530) take that path. Release each with
// FreeHostBuffer; the context keeps freed buffers and hands them to later requests of a
// similar size (2 MiB granules), so page-locking is paid once, not per request.

// HostBuffer returns n bytes of pinned host memory, or nil when there is no device (read
// into a heap buffer then, as before).
func HostBuffer(n int) []byte {
	if n <= 0 || device() == nil {
		return nil
	}
	var p unsafe.Pointer
	if C.rs_host_alloc(gpuCtx, C.size_t(n), &p) != C.RS_OK {
		return nil
	}
	return unsafe.Slice((*byte)(p), n)
}

// BodyBuffer returns a pinned buffer of length size with capacity for the profile's n
// shards, n * ceil(size/k) bytes: read the upload body into it and pass it to Encode,
// whose Split (split below, as upstream's codec.go:31) then lays the data shards and the
// parity inside the one pinned allocation. nil when there is no device or the profile
// takes the CPU codec (k+m > 256).
func BodyBuffer(size int, profile ErasureProfile) []byte {
	k, m := profile.DataShards, profile.ParityShards
	if k < 1 || m < 1 || k+m > 256 || size <= 0 {
		return nil
	}
	S := (size + k - 1) / k
	b := HostBuffer((k + m) * S)
	if b == nil {
		return nil
	}
	return b[:size]
}

// FreeHostBuffer releases a HostBuffer or BodyBuffer (any reslice of it that starts at its
// first byte). A nil or heap slice is ignored.
func FreeHostBuffer(b []byte) {
	if cap(b) == 0 || gpuCtx == nil {
		return
	}
	C.rs_host_free(gpuCtx, unsafe.Pointer(unsafe.SliceData(b)))
}

// cArray is n pointer-sized C slots (cgo: a Go []*T passed to C may not hold Go
// pointers; a C array may, while each pointee is pinned).
type cArray struct {
	base unsafe.Pointer
	n    int
}

func newCArray(n int) cArray {
	return cArray{C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))), n}
}

func (a cArray) set(i int, p unsafe.Pointer) {
	*(*unsafe.Pointer)(unsafe.Add(a.base, i*int(unsafe.Sizeof(uintptr(0))))) = p
}

func (a cArray) at(i int) **C.uint8_t {
	return (**C.uint8_t)(unsafe.Add(a.base, i*int(unsafe.Sizeof(uintptr(0)))))
}

func (a cArray) free() { C.free(a.base) }

// Encode: Split in Go with upstream's aliasing and spare-capacity reuse (split below),
// parity on the GPU (rs_encode, codec.go:36). The object is never copied into a second
// host buffer.
func (c *Codec) Encode(data []byte, profile ErasureProfile) ([][]byte, error) {
	k, m := profile.DataShards, profile.ParityShards
	if k < 1 || m < 1 {
		return nil, ErrInvalidProfile // identity, codec_test.go:113,118
	}
	// Leopard GF(2^16) profiles, no device, or an object too small to amortise the
	// ~25 µs GPU round trip: the reference codec. (Empty objects fail in its Split with
	// the same wrapped error as here, whatever k+m is.)
	if k+m > 256 || len(data) < gpuMinBytes || len(data) == 0 || device() == nil {
		return c.cpuEncode(data, profile)
	}
	shards := split(data, k, m)
	S, n := len(shards[0]), k+m
	ptrs := newCArray(n)
	defer ptrs.free()
	var pin runtime.Pinner
	defer pin.Unpin()
	for i, s := range shards {
		pin.Pin(&s[0])
		ptrs.set(i, unsafe.Pointer(&s[0]))
	}
	if rc := C.rs_encode(gpuCtx, C.int(k), C.int(m), C.size_t(S), ptrs.at(0), ptrs.at(k)); rc != C.RS_OK {
		return nil, fmt.Errorf("erasure: failed to encode parity: %w", upstreamErr(rc))
	}
	return shards, nil
}

// split lays out the n shards as upstream Split does (codec.go:31): S = ceil(len/k);
// spare capacity of data (up to n*S bytes) is zeroed past len and used in place;
// every shard lying entirely inside that extent is a sub-slice of data (the parity too
// when the capacity reaches it), and the rest are fresh zeroed buffers that receive
// the partial shard's bytes.
func split(data []byte, k, m int) [][]byte {
	n := k + m
	S := (len(data) + k - 1) / k
	need := n * S
	ext := data
	if cap(data) > len(data) {
		ext = data[:min(cap(data), need)]
		clear(ext[len(data):])
	}
	full := len(ext) / S
	shards := make([][]byte, n)
	for i := 0; i < full && i < n; i++ {
		shards[i] = ext[i*S : (i+1)*S : (i+1)*S]
	}
	if full < n {
		pad := make([]byte, (n-full)*S)
		copy(pad, ext[full*S:]) // the partial shard (zeros past len(data) stay zero)
		for i := full; i < n; i++ {
			shards[i] = pad[(i-full)*S : (i-full+1)*S : (i-full+1)*S]
		}
	}
	return shards
}

// Decode: Reconstruct + Verify + join + trim in one call (rs_codec_decode).
//
// Like upstream Reconstruct, nil or empty entries of shards are filled with the
// reconstructed shards (reusing an entry's capacity when it holds S bytes). They are
// filled only once Reconstruct has succeeded: the buffers are prepared in a private
// copy of the slice and handed over after the call, so a call failing with
// ErrTooFewShards / ErrShardSize / ErrShardNoData leaves the caller's slice exactly as
// it was (codec_test.go:65-88).
func (c *Codec) Decode(shards [][]byte, profile ErasureProfile, originalSize int64) ([]byte, error) {
	return c.decode(shards, profile, originalSize, false, false)
}

// DecodeData is Decode for callers that keep the joined object alone (RetrieveFile,
// manager.go:250-320): rs_codec_decode_data, upstream ReconstructData in Reconstruct's
// place. Missing data shards are rebuilt, filled and joined; missing parity shards stay nil
// and get no buffer; the present shards beyond the first k are verified as in Decode, and
// the errors are Decode's. An object whose k data shards are all present and that has
// nothing to verify costs a copy and no GPU work. Not in the reference API.
func (c *Codec) DecodeData(shards [][]byte, profile ErasureProfile, originalSize int64) ([]byte, error) {
	return c.decode(shards, profile, originalSize, false, true)
}

// DecodePinned is Decode for shards fetched into HostBuffers (manager.go:473,530 reading
// into HostBuffer(S) instead of io.ReadAll): the reconstructed entries it fills and the
// object it returns are HostBuffers too, so the whole call runs zero-copy. The caller
// releases the returned object and every shard entry with FreeHostBuffer once the response
// is written -- on the ErrShardCorrupted and ErrInsufficientShards paths as well: there
// Reconstruct has run and the nil entries are filled with HostBuffers, as upstream fills
// them (codec.go:55), so the caller owns and frees them. Every other error leaves the
// caller's slice untouched and frees what the call allocated. Without a device it is
// Decode (heap buffers, FreeHostBuffer ignores them).
// Not in the reference API: an addition for servers that read into pinned buffers.
func (c *Codec) DecodePinned(shards [][]byte, profile ErasureProfile, originalSize int64) ([]byte, error) {
	return c.decode(shards, profile, originalSize, true, false)
}

func (c *Codec) decode(shards [][]byte, profile ErasureProfile, originalSize int64, pinned, dataOnly bool) ([]byte, error) {
	k, m := profile.DataShards, profile.ParityShards
	if k < 1 || m < 1 {
		return nil, ErrInvalidProfile
	}
	n := k + m
	if n > 256 || originalSize < int64(gpuMinBytes) || device() == nil {
		if dataOnly {
			return cpuDecodeData(shards, profile, originalSize)
		}
		return c.cpuDecode(shards, profile, originalSize)
	}
	alloc := func(size int) []byte { return make([]byte, size) }
	var owned [][]byte // HostBuffers this call allocated, released unless handed over
	if pinned {
		alloc = func(size int) []byte {
			if b := HostBuffer(size); b != nil {
				owned = append(owned, b)
				return b
			}
			return make([]byte, size)
		}
	}
	if len(shards) != n {
		return nil, fmt.Errorf("erasure: reconstruction failed: %w", reedsolomon.ErrTooFewShards)
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
	lens := (*C.size_t)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(C.size_t(0)))))
	defer C.free(unsafe.Pointer(lens))
	lensAt := func(i int) *C.size_t {
		return (*C.size_t)(unsafe.Add(unsafe.Pointer(lens), i*int(unsafe.Sizeof(C.size_t(0)))))
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	for i := range bufs {
		*lensAt(i) = C.size_t(len(bufs[i]))
		if len(bufs[i]) == 0 && S > 0 && (i < k || !dataOnly) {
			if cap(bufs[i]) >= S {
				bufs[i] = bufs[i][:S]
			} else {
				bufs[i] = alloc(S)
			}
		}
		if len(bufs[i]) > 0 {
			pin.Pin(&bufs[i][0])
			ptrs.set(i, unsafe.Pointer(&bufs[i][0]))
		}
	}
	buf := alloc(int(originalSize))
	var out *C.uint8_t
	if originalSize > 0 {
		pin.Pin(&buf[0])
		out = (*C.uint8_t)(unsafe.Pointer(&buf[0]))
	}
	var rc C.int
	if dataOnly {
		rc = C.rs_codec_decode_data(gpuCtx, C.int(k), C.int(m), ptrs.at(0), lens, out, C.int64_t(originalSize))
	} else {
		rc = C.rs_codec_decode(gpuCtx, C.int(k), C.int(m), ptrs.at(0), lens, out, C.int64_t(originalSize))
	}
	handed := map[*byte]bool{}
	switch rc {
	case C.RS_OK, C.RS_E_CORRUPT, C.RS_E_INSUFFICIENT:
		// Reconstruct ran: upstream has filled the nil entries by now (codec.go:55); with
		// dataOnly the rebuilt ones are those whose length the call set
		for i := range shards {
			if len(shards[i]) == 0 && *lensAt(i) != 0 {
				shards[i] = bufs[i]
				handed[unsafe.SliceData(bufs[i])] = true
			}
		}
	}
	if rc == C.RS_OK {
		handed[unsafe.SliceData(buf)] = true
	}
	for _, b := range owned { // pinned buffers the caller did not receive
		if !handed[unsafe.SliceData(b)] {
			FreeHostBuffer(b)
		}
	}
	if rc != C.RS_OK {
		return nil, decodeErr(rc)
	}
	return buf, nil
}

// RepairBatch reconstructs the missing shards of many objects in one call
// (rs_reconstruct_batch), e.g. every object that lost a shard with a node. objs[b] is
// object b's n shards (nil or empty = missing). Each object's missing entries are
// filled only when that object succeeded; errs[b] is what Decode would report for it
// (Verify of the present parity beyond the first k included). Not in the reference
// API: an addition for bulk callers, no existing caller changes.
func (c *Codec) RepairBatch(objs [][][]byte, profile ErasureProfile) []error {
	return c.RepairSome(objs, nil, profile)
}

// RepairSome is RepairBatch for callers that want some shards back, not all (upstream
// ReconstructSome; rs_reconstruct_some_batch): a repair job after a dead instance fetches k
// shards per object and wants the one shard index that instance held. want[b] has n flags
// naming the entries of objs[b] to rebuild; want == nil or want[b] == nil means every missing
// entry. Entries that are missing and not wanted stay nil: no buffer, no write. Verify of the
// present shards beyond the first k and the errors are RepairBatch's. Not in the reference API.
func (c *Codec) RepairSome(objs [][][]byte, want [][]bool, profile ErasureProfile) []error {
	k, m := profile.DataShards, profile.ParityShards
	errs := make([]error, len(objs))
	wanted := func(b, i int) bool {
		return want == nil || b >= len(want) || want[b] == nil || (i < len(want[b]) && want[b][i])
	}
	if k < 1 || m < 1 {
		for b := range errs {
			errs[b] = ErrInvalidProfile
		}
		return errs
	}
	n := k + m
	if len(objs) == 0 {
		return errs
	}
	if n > 256 || device() == nil {
		for b, shards := range objs {
			if want == nil || b >= len(want) || want[b] == nil {
				errs[b] = cpuRepair(shards, k, m)
			} else {
				errs[b] = cpuRepairSome(shards, want[b], k, m)
			}
		}
		return errs
	}
	bufs := make([][][]byte, len(objs))
	ptrs := newCArray(len(objs) * n)
	defer ptrs.free()
	lens := make([]C.size_t, len(objs)*n) // Go memory without Go pointers: may be passed
	req := make([]C.uint8_t, len(objs)*n)
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
			if wanted(b, i) {
				req[b*n+i] = 1
			}
			if len(s) == 0 && S > 0 && wanted(b, i) {
				s = make([]byte, S)
				bufs[b][i] = s
			}
			if len(s) > 0 {
				pin.Pin(&s[0])
				ptrs.set(b*n+i, unsafe.Pointer(&s[0]))
			}
		}
	}
	rc := C.rs_reconstruct_some_batch(gpuCtx, C.int(k), C.int(m), C.int(len(objs)), ptrs.at(0),
		&lens[0], &req[0], 1, &status[0])
	stripeArg := false // RS_E_ARG is per-stripe only when some stripe reports it
	for _, st := range status {
		stripeArg = stripeArg || st == C.RS_E_ARG
	}
	switch {
	case rc == C.RS_OK, rc == C.RS_E_CORRUPT, rc == C.RS_E_TOO_FEW_SHARDS,
		rc == C.RS_E_SHARD_SIZE, rc == C.RS_E_NO_DATA, rc == C.RS_E_ARG && stripeArg:
		// per-stripe statuses are valid (RS_E_ARG: a stripe with a nil present entry)
	default: // a call-level error: no status was written
		for b := range errs {
			if errs[b] == nil {
				errs[b] = decodeErr(rc)
			}
		}
		return errs
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
			}
		}
		errs[b] = decodeErr(st)
	}
	return errs
}

// EncodeBatch is Encode for many objects of one profile in one call
// (rs_codec_encode_batch: one pipeline over all of them, Split done on the way into its
// staging; DESIGN.md §7.6), e.g. a server batching small uploads. out[b] holds object b's
// n shards and errs[b] what Encode would report for it. An object whose capacity holds all
// n shards (a BodyBuffer) is split in place as Encode splits it; any other object gets one
// fresh buffer of n*S bytes that holds all its shards, so unlike upstream Split no shard
// aliases objs[b]. The batch goes to the GPU whatever the objects' sizes (gpuMinBytes is
// the single-object threshold). Not in the reference API: an addition for bulk callers.
func (c *Codec) EncodeBatch(objs [][]byte, profile ErasureProfile) ([][][]byte, []error) {
	k, m := profile.DataShards, profile.ParityShards
	out := make([][][]byte, len(objs))
	errs := make([]error, len(objs))
	if k < 1 || m < 1 {
		for b := range errs {
			errs[b] = ErrInvalidProfile
		}
		return out, errs
	}
	if len(objs) == 0 {
		return out, errs
	}
	n := k + m
	if n > 256 || device() == nil {
		for b, d := range objs {
			out[b], errs[b] = c.cpuEncode(d, profile)
		}
		return out, errs
	}
	B := len(objs)
	data, dst := newCArray(B), newCArray(B)
	defer data.free()
	defer dst.free()
	lens := make([]C.size_t, B) // Go memory without Go pointers: may be passed
	caps := make([]C.size_t, B)
	sizes := make([]C.size_t, B)
	status := make([]C.int, B)
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
	rc := C.rs_codec_encode_batch(gpuCtx, C.int(k), C.int(m), C.int(B), data.at(0), &lens[0],
		dst.at(0), &caps[0], &sizes[0], &status[0])
	if rc != C.RS_OK && !hasStatus(status, rc) { // a call-level error: no status was written
		for b := range errs {
			errs[b] = fmt.Errorf("erasure: failed to encode parity: %w", upstreamErr(rc))
		}
		return out, errs
	}
	for b := range objs {
		switch st := status[b]; st {
		case C.RS_OK:
			S := int(sizes[b])
			out[b] = make([][]byte, n)
			for i := range out[b] {
				out[b][i] = bufs[b][i*S : (i+1)*S : (i+1)*S]
			}
		case C.RS_E_SHORT_DATA:
			errs[b] = fmt.Errorf("erasure: failed to split data: %w", upstreamErr(st))
		default:
			errs[b] = fmt.Errorf("erasure: failed to encode parity: %w", upstreamErr(st))
		}
	}
	return out, errs
}

// hasStatus: a batch call returns the first nonzero per-object status, so a return value no
// object reports is a call-level error.
func hasStatus(status []C.int, rc C.int) bool {
	for _, st := range status {
		if st == rc {
			return true
		}
	}
	return false
}

// DecodeBatch is Decode for many objects of one profile in one call
// (rs_codec_decode_batch: Reconstruct, Verify and the join / trim of every object in one
// pipeline). shards[b] is object b's n shards (nil or empty = missing), sizes[b] its
// original size; out[b] is the object and errs[b] what Decode would report for it. Like
// Decode, an object's missing entries are filled once its Reconstruct has run
// (errs[b] nil, ErrShardCorrupted or ErrInsufficientShards) and left alone otherwise. Not in
// the reference API: an addition for bulk callers.
func (c *Codec) DecodeBatch(shards [][][]byte, profile ErasureProfile, sizes []int64) ([][]byte, []error) {
	return c.decodeBatch(shards, profile, sizes, false)
}

// DecodeDataBatch is DecodeData for many objects of one profile in one call
// (rs_codec_decode_data_batch): DecodeBatch that rebuilds and fills missing data shards
// alone. Objects that need no row at all are joined by a copy, and a batch of such objects
// reaches no device. Not in the reference API.
func (c *Codec) DecodeDataBatch(shards [][][]byte, profile ErasureProfile, sizes []int64) ([][]byte, []error) {
	return c.decodeBatch(shards, profile, sizes, true)
}

func (c *Codec) decodeBatch(shards [][][]byte, profile ErasureProfile, sizes []int64, dataOnly bool) ([][]byte, []error) {
	k, m := profile.DataShards, profile.ParityShards
	out := make([][]byte, len(shards))
	errs := make([]error, len(shards))
	if k < 1 || m < 1 || len(sizes) != len(shards) {
		for b := range errs {
			errs[b] = ErrInvalidProfile
			if k >= 1 && m >= 1 {
				errs[b] = fmt.Errorf("erasure: %d sizes for %d objects", len(sizes), len(shards))
			}
		}
		return out, errs
	}
	if len(shards) == 0 {
		return out, errs
	}
	n := k + m
	if n > 256 || device() == nil {
		for b := range shards {
			if dataOnly {
				out[b], errs[b] = cpuDecodeData(shards[b], profile, sizes[b])
			} else {
				out[b], errs[b] = c.cpuDecode(shards[b], profile, sizes[b])
			}
		}
		return out, errs
	}
	B := len(shards)
	bufs := make([][][]byte, B)
	ptrs, outs := newCArray(B*n), newCArray(B)
	defer ptrs.free()
	defer outs.free()
	lens := make([]C.size_t, B*n) // Go memory without Go pointers: may be passed
	osz := make([]C.int64_t, B)
	status := make([]C.int, B)
	var pin runtime.Pinner
	defer pin.Unpin()
	for b, sh := range shards {
		if len(sh) != n {
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
			if len(s) == 0 && S > 0 && (i < k || !dataOnly) {
				if cap(s) >= S {
					s = s[:S]
				} else {
					s = make([]byte, S)
				}
				bufs[b][i] = s
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
	var rc C.int
	if dataOnly {
		rc = C.rs_codec_decode_data_batch(gpuCtx, C.int(k), C.int(m), C.int(B), ptrs.at(0), &lens[0],
			outs.at(0), &osz[0], &status[0])
	} else {
		rc = C.rs_codec_decode_batch(gpuCtx, C.int(k), C.int(m), C.int(B), ptrs.at(0), &lens[0],
			outs.at(0), &osz[0], &status[0])
	}
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
		switch st {
		case C.RS_OK, C.RS_E_CORRUPT, C.RS_E_INSUFFICIENT:
			// Reconstruct ran: upstream has filled the nil entries by now (codec.go:55)
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
	return out, errs
}

// cpuRepair is RepairBatch's per-object CPU form: upstream Reconstruct + Verify.
func cpuRepair(shards [][]byte, k, m int) error {
	enc, err := reedsolomon.New(k, m)
	if err != nil {
		return fmt.Errorf("erasure: failed to create decoder: %w", err)
	}
	if err := enc.Reconstruct(shards); err != nil {
		return fmt.Errorf("erasure: reconstruction failed: %w", err)
	}
	ok, err := enc.Verify(shards)
	if err != nil {
		return fmt.Errorf("erasure: verification failed: %w", err)
	}
	if !ok {
		return ErrShardCorrupted
	}
	return nil
}

// ---- parity updated in place (upstream Update / EncodeIdx; DESIGN.md §5.11) -------------

// updateErr maps the codes of the update calls: the erasure sentinels by identity, anything
// upstream Update would have reported inside Encode's wrapper.
func updateErr(rc C.int) error {
	switch rc {
	case C.RS_OK:
		return nil
	case C.RS_E_INVALID_PROFILE:
		return ErrInvalidProfile
	case C.RS_E_ARG:
		return fmt.Errorf("erasure: failed to update parity: %w", reedsolomon.ErrInvalidInput)
	}
	return fmt.Errorf("erasure: failed to update parity: %w", upstreamErr(rc))
}

// checkUpdate is upstream Update's argument check, in its order: the shard counts, a changed
// shard without its old bytes (ErrInvalidInput), then the sizes. Returns the shard size.
func checkUpdate(shards, newData [][]byte, k, m int) (int, error) {
	wrap := func(err error) error { return fmt.Errorf("erasure: failed to update parity: %w", err) }
	if len(shards) != k+m || len(newData) != k {
		return 0, wrap(reedsolomon.ErrTooFewShards)
	}
	S := 0
	for i, nd := range newData {
		if nd != nil && shards[i] == nil {
			return 0, wrap(reedsolomon.ErrInvalidInput)
		}
	}
	for _, s := range shards {
		if len(s) > 0 {
			S = len(s)
			break
		}
	}
	if S == 0 {
		return 0, wrap(reedsolomon.ErrShardNoData)
	}
	for i, s := range shards {
		if (i >= k || newData[i] != nil) && len(s) != S {
			return 0, wrap(reedsolomon.ErrShardSize)
		}
	}
	for _, nd := range newData {
		if nd != nil && len(nd) != S {
			return 0, wrap(reedsolomon.ErrShardSize)
		}
	}
	return S, nil
}

// UpdateParity is upstream enc.Update(shards, newData) (rs_update): shards holds the old data
// shards -- only those that changed are read, the others may be nil -- and the m parity
// shards, which are updated in place; newData has k entries, nil = unchanged. The data entries
// of shards stay as they are. An update of c shards moves (2c+2m)*S bytes where a full Encode
// moves (k+m)*S and needs all k data shards. Not in the reference API.
func (c *Codec) UpdateParity(shards, newData [][]byte, profile ErasureProfile) error {
	k, m := profile.DataShards, profile.ParityShards
	if k < 1 || m < 1 {
		return ErrInvalidProfile
	}
	if k+m > 256 || device() == nil {
		return cpuUpdateParity(shards, newData, k, m)
	}
	S, err := checkUpdate(shards, newData, k, m)
	if err != nil {
		return err
	}
	olds, news, par := newCArray(k), newCArray(k), newCArray(m)
	defer olds.free()
	defer news.free()
	defer par.free()
	var pin runtime.Pinner
	defer pin.Unpin()
	for i, nd := range newData {
		if nd == nil {
			continue
		}
		pin.Pin(&nd[0])
		pin.Pin(&shards[i][0])
		news.set(i, unsafe.Pointer(&nd[0]))
		olds.set(i, unsafe.Pointer(&shards[i][0]))
	}
	for j := 0; j < m; j++ {
		pin.Pin(&shards[k+j][0])
		par.set(j, unsafe.Pointer(&shards[k+j][0]))
	}
	return updateErr(C.rs_update(gpuCtx, C.int(k), C.int(m), C.size_t(S), olds.at(0), news.at(0), par.at(0)))
}

// EncodeIdx is upstream enc.EncodeIdx(dataShard, idx, parity) (rs_encode_idx): it adds data
// shard idx's contribution to the m parity shards in place. Zero the parity before the first
// shard; the k shards may then arrive in any order. Not in the reference API.
func (c *Codec) EncodeIdx(dataShard []byte, idx int, parity [][]byte, profile ErasureProfile) error {
	k, m := profile.DataShards, profile.ParityShards
	if k < 1 || m < 1 {
		return ErrInvalidProfile
	}
	if k+m > 256 || device() == nil {
		return cpuEncodeIdx(dataShard, idx, parity, k, m)
	}
	wrap := func(err error) error { return fmt.Errorf("erasure: failed to update parity: %w", err) }
	// upstream's order: the parity count, the index, then the sizes
	if len(parity) != m {
		return wrap(reedsolomon.ErrTooFewShards)
	}
	if idx < 0 || idx >= k {
		return wrap(reedsolomon.ErrInvalidShardIdx)
	}
	if len(dataShard) == 0 {
		return wrap(reedsolomon.ErrShardNoData)
	}
	par := newCArray(m)
	defer par.free()
	var pin runtime.Pinner
	defer pin.Unpin()
	for j, p := range parity {
		if len(p) != len(dataShard) {
			return wrap(reedsolomon.ErrShardSize)
		}
		pin.Pin(&p[0])
		par.set(j, unsafe.Pointer(&p[0]))
	}
	pin.Pin(&dataShard[0])
	return updateErr(C.rs_encode_idx(gpuCtx, C.int(k), C.int(m), C.size_t(len(dataShard)),
		(*C.uint8_t)(unsafe.Pointer(&dataShard[0])), C.int(idx), par.at(0)))
}

// UpdateBatch is UpdateParity for many stripes of one profile in one call (rs_update_batch:
// one pipeline over all of them, whatever their sizes and changed sets). shards[b] and
// newData[b] are stripe b's arguments to UpdateParity; errs[b] is what it would report.
func (c *Codec) UpdateBatch(shards, newData [][][]byte, profile ErasureProfile) []error {
	k, m := profile.DataShards, profile.ParityShards
	errs := make([]error, len(shards))
	if len(newData) != len(shards) {
		for b := range errs {
			errs[b] = fmt.Errorf("erasure: %d new-data rows for %d stripes", len(newData), len(shards))
		}
		return errs
	}
	if k < 1 || m < 1 {
		for b := range errs {
			errs[b] = ErrInvalidProfile
		}
		return errs
	}
	if len(shards) == 0 {
		return errs
	}
	if k+m > 256 || device() == nil {
		for b := range shards {
			errs[b] = cpuUpdateParity(shards[b], newData[b], k, m)
		}
		return errs
	}
	B := len(shards)
	olds, news, par := newCArray(B*k), newCArray(B*k), newCArray(B*m)
	defer olds.free()
	defer news.free()
	defer par.free()
	sizes := make([]C.size_t, B)
	status := make([]C.int, B)
	var pin runtime.Pinner
	defer pin.Unpin()
	for b := range shards {
		S, err := checkUpdate(shards[b], newData[b], k, m)
		if err != nil {
			errs[b] = err
			continue // no pointers: the stripe has no change for the library
		}
		sizes[b] = C.size_t(S)
		for i, nd := range newData[b] {
			if nd == nil {
				continue
			}
			pin.Pin(&nd[0])
			pin.Pin(&shards[b][i][0])
			news.set(b*k+i, unsafe.Pointer(&nd[0]))
			olds.set(b*k+i, unsafe.Pointer(&shards[b][i][0]))
		}
		for j := 0; j < m; j++ {
			pin.Pin(&shards[b][k+j][0])
			par.set(b*m+j, unsafe.Pointer(&shards[b][k+j][0]))
		}
	}
	rc := C.rs_update_batch(gpuCtx, C.int(k), C.int(m), C.int(B), &sizes[0], olds.at(0), news.at(0),
		par.at(0), &status[0])
	if rc != C.RS_OK && !hasStatus(status, rc) { // a call-level error: no status was written
		for b := range errs {
			if errs[b] == nil {
				errs[b] = updateErr(rc)
			}
		}
		return errs
	}
	for b := range errs {
		if errs[b] == nil {
			errs[b] = updateErr(status[b])
		}
	}
	return errs
}

// ---- progressive decode (upstream DecodeIdx; DESIGN.md §5.14) ---------------------------

// decodeIdxErr maps the codes of the decode-idx calls as updateErr does, inside Decode's wrapper.
func decodeIdxErr(rc C.int) error {
	switch rc {
	case C.RS_OK:
		return nil
	case C.RS_E_INVALID_PROFILE:
		return ErrInvalidProfile
	case C.RS_E_ARG:
		return fmt.Errorf("erasure: failed to decode: %w", reedsolomon.ErrInvalidInput)
	}
	return fmt.Errorf("erasure: failed to decode: %w", upstreamErr(rc))
}

// checkDecodeIdx checks one stripe's argument counts and sizes: k+m entries each, one size over
// every given dst and input. The expect count and the misplaced entries are the library's to
// refuse (RS_E_TOO_FEW_SHARDS, RS_E_ARG). Returns the shard size (0: nothing given).
func checkDecodeIdx(dst [][]byte, expectInput []bool, input [][]byte, k, m int) (int, error) {
	wrap := func(err error) error { return fmt.Errorf("erasure: failed to decode: %w", err) }
	if len(dst) != k+m || len(expectInput) != k+m || len(input) != k+m {
		return 0, wrap(reedsolomon.ErrTooFewShards)
	}
	S := 0
	for _, rows := range [][][]byte{dst, input} {
		for _, s := range rows {
			if len(s) == 0 {
				continue
			}
			if S == 0 {
				S = len(s)
			}
			if len(s) != S {
				return 0, wrap(reedsolomon.ErrShardSize)
			}
		}
	}
	return S, nil
}

// DecodeIdx is upstream enc.DecodeIdx(dst, expectInput, input) (rs_decode_idx), the decode twin
// of EncodeIdx: expectInput (k+m flags, exactly k set) fixes the shards the decode will be fed
// over all calls, input (k+m entries, nil = not delivered with this call) holds the shards that
// have arrived, dst (k+m entries, nil = not wanted) the shards to rebuild, at indices that are
// not expected. The delivered shards' contribution is added into every wanted shard. Zero dst
// before the first call; once every expected shard has been delivered, in any order, dst holds
// what Reconstruct gives from those k shards. Each call pays its own round trip to the device.
// Not in the reference API.
func (c *Codec) DecodeIdx(dst [][]byte, expectInput []bool, input [][]byte, profile ErasureProfile) error {
	errs := c.DecodeIdxBatch([][][]byte{dst}, [][]bool{expectInput}, [][][]byte{input}, profile)
	return errs[0]
}

// DecodeIdxBatch is DecodeIdx for many stripes of one profile in one call (rs_decode_idx_batch:
// one pipeline over all of them, whatever their sizes, expected sets, wanted sets and delivered
// shards). dst[b], expectInput[b] and input[b] are stripe b's arguments to DecodeIdx; errs[b]
// is what it would report.
func (c *Codec) DecodeIdxBatch(dst [][][]byte, expectInput [][]bool, input [][][]byte, profile ErasureProfile) []error {
	k, m := profile.DataShards, profile.ParityShards
	errs := make([]error, len(dst))
	if len(expectInput) != len(dst) || len(input) != len(dst) {
		for b := range errs {
			errs[b] = fmt.Errorf("erasure: %d expect rows and %d input rows for %d stripes", len(expectInput),
				len(input), len(dst))
		}
		return errs
	}
	if k < 1 || m < 1 {
		for b := range errs {
			errs[b] = ErrInvalidProfile
		}
		return errs
	}
	if len(dst) == 0 {
		return errs
	}
	if k+m > 256 || device() == nil {
		for b := range dst {
			errs[b] = cpuDecodeIdx(dst[b], expectInput[b], input[b], k, m)
		}
		return errs
	}
	B, n := len(dst), k+m
	ins, outs := newCArray(B*n), newCArray(B*n)
	defer ins.free()
	defer outs.free()
	sizes := make([]C.size_t, B)
	status := make([]C.int, B)
	expect := make([]C.uint8_t, B*n)
	var pin runtime.Pinner
	defer pin.Unpin()
	for b := range dst {
		S, err := checkDecodeIdx(dst[b], expectInput[b], input[b], k, m)
		if err != nil {
			errs[b] = err
			for i := 0; i < k && i < n; i++ { // a well-formed stripe with nothing to do for the library
				expect[b*n+i] = 1
			}
			continue
		}
		sizes[b] = C.size_t(S)
		for i := 0; i < n; i++ {
			if expectInput[b][i] {
				expect[b*n+i] = 1
			}
			if len(input[b][i]) > 0 {
				pin.Pin(&input[b][i][0])
				ins.set(b*n+i, unsafe.Pointer(&input[b][i][0]))
			}
			if len(dst[b][i]) > 0 {
				pin.Pin(&dst[b][i][0])
				outs.set(b*n+i, unsafe.Pointer(&dst[b][i][0]))
			}
		}
	}
	rc := C.rs_decode_idx_batch(gpuCtx, C.int(k), C.int(m), C.int(B), &sizes[0], outs.at(0), &expect[0],
		ins.at(0), 0, &status[0])
	if rc != C.RS_OK && !hasStatus(status, rc) { // a call-level error: no status was written
		for b := range errs {
			if errs[b] == nil {
				errs[b] = decodeIdxErr(rc)
			}
		}
		return errs
	}
	for b := range errs {
		if errs[b] == nil {
			errs[b] = decodeIdxErr(status[b])
		}
	}
	return errs
}

// ---- progressive Verify (DESIGN.md §5.15) ------------------------------------------------

// DecodeCheck is DecodeIdx that also checks the shards fetched beyond the k expected ones
// (rs_decode_check): check (k+m entries, nil = not compared) holds one syndrome accumulator per
// compared shard, at indices that are neither expected nor wanted, zeroed before the first call;
// input may then deliver the compared shard itself. Every call adds the delivered expected
// shards' terms, and the compared shard when it arrives, into its accumulator. A final call
// writes no accumulator: it tests the value each would have received and returns
// ErrShardCorrupted when a byte of it is nonzero -- after the wanted shards have been written,
// as Decode's Verify fails after Reconstruct. RetrieveFile with DecodeCheck is Decode, Verify
// included. Not in the reference API.
func (c *Codec) DecodeCheck(dst, check [][]byte, expectInput []bool, input [][]byte, final bool, profile ErasureProfile) error {
	errs := c.DecodeCheckBatch([][][]byte{dst}, [][][]byte{check}, [][]bool{expectInput}, [][][]byte{input}, final, profile)
	return errs[0]
}

// DecodeCheckBatch is DecodeCheck for many stripes of one profile in one call
// (rs_decode_check_batch); errs[b] is what DecodeCheck would report for stripe b.
func (c *Codec) DecodeCheckBatch(dst, check [][][]byte, expectInput [][]bool, input [][][]byte, final bool, profile ErasureProfile) []error {
	k, m := profile.DataShards, profile.ParityShards
	errs := make([]error, len(dst))
	if len(check) != len(dst) || len(expectInput) != len(dst) || len(input) != len(dst) {
		for b := range errs {
			errs[b] = fmt.Errorf("erasure: %d check rows, %d expect rows and %d input rows for %d stripes", len(check),
				len(expectInput), len(input), len(dst))
		}
		return errs
	}
	if k < 1 || m < 1 {
		for b := range errs {
			errs[b] = ErrInvalidProfile
		}
		return errs
	}
	if len(dst) == 0 {
		return errs
	}
	if k+m > 256 || device() == nil {
		for b := range dst {
			errs[b] = cpuDecodeCheck(dst[b], check[b], expectInput[b], input[b], final, k, m)
		}
		return errs
	}
	B, n := len(dst), k+m
	ins, outs, accs := newCArray(B*n), newCArray(B*n), newCArray(B*n)
	defer ins.free()
	defer outs.free()
	defer accs.free()
	sizes := make([]C.size_t, B)
	status := make([]C.int, B)
	expect := make([]C.uint8_t, B*n)
	var pin runtime.Pinner
	defer pin.Unpin()
	for b := range dst {
		var S int
		var err error
		if len(check[b]) != n || len(dst[b]) != n {
			err = fmt.Errorf("erasure: failed to decode: %w", reedsolomon.ErrTooFewShards)
		} else {
			// the accumulators take part in the size check as the destinations do
			rows := make([][]byte, n)
			for i := range rows {
				rows[i] = dst[b][i]
				if len(check[b][i]) > 0 {
					rows[i] = check[b][i]
				}
			}
			S, err = checkDecodeIdx(rows, expectInput[b], input[b], k, m)
		}
		if err != nil {
			errs[b] = err
			for i := 0; i < k && i < n; i++ { // a well-formed stripe with nothing to do for the library
				expect[b*n+i] = 1
			}
			continue
		}
		sizes[b] = C.size_t(S)
		for i := 0; i < n; i++ {
			if expectInput[b][i] {
				expect[b*n+i] = 1
			}
			if len(input[b][i]) > 0 {
				pin.Pin(&input[b][i][0])
				ins.set(b*n+i, unsafe.Pointer(&input[b][i][0]))
			}
			if len(dst[b][i]) > 0 {
				pin.Pin(&dst[b][i][0])
				outs.set(b*n+i, unsafe.Pointer(&dst[b][i][0]))
			}
			if len(check[b][i]) > 0 {
				pin.Pin(&check[b][i][0])
				accs.set(b*n+i, unsafe.Pointer(&check[b][i][0]))
			}
		}
	}
	flags := C.uint(0)
	if final {
		flags = C.RS_DECODE_CHECK_FINAL
	}
	rc := C.rs_decode_check_batch(gpuCtx, C.int(k), C.int(m), C.int(B), &sizes[0], outs.at(0), accs.at(0), &expect[0],
		ins.at(0), flags, &status[0])
	if rc != C.RS_OK && !hasStatus(status, rc) { // a call-level error: no status was written
		for b := range errs {
			if errs[b] == nil {
				errs[b] = decodeIdxErr(rc)
			}
		}
		return errs
	}
	for b := range errs {
		if errs[b] == nil {
			if status[b] == C.RS_E_CORRUPT {
				errs[b] = ErrShardCorrupted
			} else {
				errs[b] = decodeIdxErr(status[b])
			}
		}
	}
	return errs
}

// ---- progressive repair (DESIGN.md §5.16) ------------------------------------------------

// DecodeRepair is the final DecodeCheck call that repairs what it flags (rs_decode_repair): dst,
// check, expectInput and input as DecodeCheck takes them; fix (k+m entries, nil = none) holds
// buffers at expected or compared indices into which the shard's error values are XORed -- a
// zeroed buffer ends as the error row, the shard as delivered ends restored, and fix[i] may be
// input[i]. With three or more compared shards a single corrupt shard per byte column is taken
// out of the wanted shards and named: counts[i] is the number of columns blamed on shard i,
// counts[k+m] the number left unexplained. A stripe with an unexplained column returns
// ErrShardCorrupted after the wanted shards have been written, as DecodeCheck does. Like the
// rest of this package it has never been compiled where the library is developed. Not in the
// reference API.
func (c *Codec) DecodeRepair(dst, check, fix [][]byte, expectInput []bool, input [][]byte, profile ErasureProfile) ([]uint64, error) {
	counts, errs := c.DecodeRepairBatch([][][]byte{dst}, [][][]byte{check}, [][][]byte{fix}, [][]bool{expectInput},
		[][][]byte{input}, profile)
	return counts[0], errs[0]
}

// DecodeRepairBatch is DecodeRepair for many stripes of one profile in one call
// (rs_decode_repair_batch); counts[b] and errs[b] are what DecodeRepair would report for stripe b.
func (c *Codec) DecodeRepairBatch(dst, check, fix [][][]byte, expectInput [][]bool, input [][][]byte, profile ErasureProfile) ([][]uint64, []error) {
	k, m := profile.DataShards, profile.ParityShards
	errs := make([]error, len(dst))
	counts := make([][]uint64, len(dst))
	if len(check) != len(dst) || len(fix) != len(dst) || len(expectInput) != len(dst) || len(input) != len(dst) {
		for b := range errs {
			errs[b] = fmt.Errorf("erasure: %d check rows, %d fix rows, %d expect rows and %d input rows for %d stripes",
				len(check), len(fix), len(expectInput), len(input), len(dst))
		}
		return counts, errs
	}
	if k < 1 || m < 1 {
		for b := range errs {
			errs[b] = ErrInvalidProfile
		}
		return counts, errs
	}
	if len(dst) == 0 {
		return counts, errs
	}
	if k+m > 256 || device() == nil {
		for b := range dst {
			counts[b], errs[b] = cpuDecodeRepair(dst[b], check[b], fix[b], expectInput[b], input[b], k, m)
		}
		return counts, errs
	}
	B, n := len(dst), k+m
	ins, outs, accs, fixes := newCArray(B*n), newCArray(B*n), newCArray(B*n), newCArray(B*n)
	defer ins.free()
	defer outs.free()
	defer accs.free()
	defer fixes.free()
	sizes := make([]C.size_t, B)
	status := make([]C.int, B)
	expect := make([]C.uint8_t, B*n)
	flat := make([]C.uint64_t, B*(n+1))
	var pin runtime.Pinner
	defer pin.Unpin()
	for b := range dst {
		var S int
		var err error
		if len(check[b]) != n || len(dst[b]) != n || len(fix[b]) != n {
			err = fmt.Errorf("erasure: failed to decode: %w", reedsolomon.ErrTooFewShards)
		} else {
			rows := make([][]byte, n)
			for i := range rows {
				rows[i] = dst[b][i]
				if len(check[b][i]) > 0 {
					rows[i] = check[b][i]
				}
			}
			S, err = checkDecodeIdx(rows, expectInput[b], input[b], k, m)
			for i := 0; err == nil && i < n; i++ {
				if len(fix[b][i]) > 0 && len(fix[b][i]) != S {
					err = fmt.Errorf("erasure: failed to decode: %w", reedsolomon.ErrShardSize)
				}
			}
		}
		if err != nil {
			errs[b] = err
			for i := 0; i < k && i < n; i++ { // a well-formed stripe with nothing to do for the library
				expect[b*n+i] = 1
			}
			continue
		}
		sizes[b] = C.size_t(S)
		for i := 0; i < n; i++ {
			if expectInput[b][i] {
				expect[b*n+i] = 1
			}
			if len(input[b][i]) > 0 {
				pin.Pin(&input[b][i][0])
				ins.set(b*n+i, unsafe.Pointer(&input[b][i][0]))
			}
			if len(dst[b][i]) > 0 {
				pin.Pin(&dst[b][i][0])
				outs.set(b*n+i, unsafe.Pointer(&dst[b][i][0]))
			}
			if len(check[b][i]) > 0 {
				pin.Pin(&check[b][i][0])
				accs.set(b*n+i, unsafe.Pointer(&check[b][i][0]))
			}
			if len(fix[b][i]) > 0 {
				pin.Pin(&fix[b][i][0])
				fixes.set(b*n+i, unsafe.Pointer(&fix[b][i][0]))
			}
		}
	}
	rc := C.rs_decode_repair_batch(gpuCtx, C.int(k), C.int(m), C.int(B), &sizes[0], outs.at(0), accs.at(0), fixes.at(0),
		&expect[0], ins.at(0), 0, &status[0], &flat[0])
	if rc != C.RS_OK && !hasStatus(status, rc) { // a call-level error: no status was written
		for b := range errs {
			if errs[b] == nil {
				errs[b] = decodeIdxErr(rc)
			}
		}
		return counts, errs
	}
	for b := range errs {
		if errs[b] != nil {
			continue
		}
		counts[b] = make([]uint64, n+1)
		for i := range counts[b] {
			counts[b][i] = uint64(flat[b*(n+1)+i])
		}
		if status[b] == C.RS_E_CORRUPT {
			errs[b] = ErrShardCorrupted
		} else {
			errs[b] = decodeIdxErr(status[b])
		}
	}
	return counts, errs
}

// ---- decode sessions (DESIGN.md §5.17) --------------------------------------------------------

// DecodeSession is a progressive decode of one object whose rows stay on the device
// (rs_session_open): Feed each shard as RetrieveFile's fetches deliver it, from any goroutine
// and in any order, then Finish for the joined, trimmed object. On a profile or a machine the
// GPU codec does not serve it collects the shards and decodes at Finish. Like the rest of this
// package it has never been compiled where the library is developed. Not in the reference API.
type DecodeSession struct {
	c       *Codec
	h       *C.rs_session
	profile ErasureProfile
	size    int64
	S       int
	want    []bool
	repair  bool
	mu      sync.Mutex
	out     []byte
	fed     [][]byte // the CPU form's shards; the GPU form's delivered data shards' indices are in out
	gotData []bool
}

// DecodeSession opens a session for an object of originalSize bytes: expect names the k shard
// indices that will be fed, compare the indices fetched beyond them, which Finish checks against
// them (with repair: and uses to repair a corrupt one, given three or more).
func (c *Codec) DecodeSession(profile ErasureProfile, originalSize int64, expect, compare []int, repair bool) (*DecodeSession, error) {
	k, m := profile.DataShards, profile.ParityShards
	if k < 1 || m < 1 {
		return nil, ErrInvalidProfile
	}
	n := k + m
	if originalSize < 0 {
		originalSize = 0
	}
	S := int((originalSize + int64(k) - 1) / int64(k))
	if S < 1 {
		S = 1
	}
	s := &DecodeSession{c: c, profile: profile, size: originalSize, S: S, repair: repair,
		want: make([]bool, n), out: make([]byte, originalSize), fed: make([][]byte, n), gotData: make([]bool, n)}
	e, w, cm := make([]C.uint8_t, n), make([]C.uint8_t, n), make([]C.uint8_t, n)
	for _, i := range expect {
		if i < 0 || i >= n {
			return nil, reedsolomon.ErrInvalidShardIdx
		}
		e[i] = 1
	}
	for _, i := range compare {
		if i < 0 || i >= n {
			return nil, reedsolomon.ErrInvalidShardIdx
		}
		cm[i] = 1
	}
	for i := 0; i < k; i++ {
		if e[i] == 0 && cm[i] == 0 {
			w[i] = 1
			s.want[i] = true
		}
	}
	if n > 256 || device() == nil {
		return s, nil
	}
	flags := C.uint(C.RS_SESSION_CHECK)
	if repair {
		flags = C.RS_SESSION_REPAIR
	}
	if rc := C.rs_session_open(gpuCtx, C.int(k), C.int(m), C.size_t(S), &e[0], &w[0], &cm[0], flags, &s.h); rc != C.RS_OK {
		return nil, decodeIdxErr(rc)
	}
	return s, nil
}

// span is where data shard i lies in the object: [a, b), empty for a shard that is all padding.
func (s *DecodeSession) span(i int) (int64, int64) {
	a, b := int64(i)*int64(s.S), int64(i+1)*int64(s.S)
	if a > s.size {
		a = s.size
	}
	if b > s.size {
		b = s.size
	}
	return a, b
}

// Feed delivers shard idx, once; it returns when shard may be reused. A delivered data shard is
// kept where it belongs in the object.
func (s *DecodeSession) Feed(idx int, shard []byte) error {
	n := s.profile.DataShards + s.profile.ParityShards
	if idx < 0 || idx >= n {
		return reedsolomon.ErrInvalidShardIdx
	}
	if len(shard) != s.S {
		return fmt.Errorf("erasure: failed to decode: %w", reedsolomon.ErrShardSize)
	}
	if s.h == nil {
		s.mu.Lock()
		defer s.mu.Unlock()
		s.fed[idx] = append([]byte(nil), shard...)
		return nil
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&shard[0])
	if rc := C.rs_session_feed(s.h, C.int(idx), (*C.uint8_t)(unsafe.Pointer(&shard[0]))); rc != C.RS_OK {
		return decodeIdxErr(rc)
	}
	if idx < s.profile.DataShards {
		a, b := s.span(idx)
		s.mu.Lock()
		copy(s.out[a:b], shard)
		s.gotData[idx] = true
		s.mu.Unlock()
	}
	return nil
}

// Finish closes the decode and returns the object. ErrShardCorrupted comes with the object's
// bytes filled in all the same, as Decode delivers them before Verify fails; before the k-th
// expected shard it is ErrTooFewShards and the session stays usable.
func (s *DecodeSession) Finish() ([]byte, error) {
	k, m := s.profile.DataShards, s.profile.ParityShards
	n := k + m
	if s.h == nil {
		s.mu.Lock()
		defer s.mu.Unlock()
		return s.c.Decode(s.fed, s.profile, s.size)
	}
	dst, fix := newCArray(n), newCArray(n)
	defer dst.free()
	defer fix.free()
	lens := make([]C.size_t, n)
	counts := make([]C.uint64_t, n+1)
	fixRows := make([][]byte, n)
	var pin runtime.Pinner
	defer pin.Unpin()
	for i := 0; i < k; i++ {
		a, b := s.span(i)
		if s.want[i] && b > a {
			pin.Pin(&s.out[a])
			dst.set(i, unsafe.Pointer(&s.out[a]))
			lens[i] = C.size_t(b - a)
		}
		if s.repair && s.gotData[i] {
			fixRows[i] = make([]byte, s.S)
			pin.Pin(&fixRows[i][0])
			fix.set(i, unsafe.Pointer(&fixRows[i][0]))
		}
	}
	var fixp **C.uint8_t
	if s.repair {
		fixp = fix.at(0)
	}
	rc := C.rs_session_finish(s.h, dst.at(0), &lens[0], fixp, &counts[0])
	if rc != C.RS_OK && rc != C.RS_E_CORRUPT {
		return nil, decodeIdxErr(rc)
	}
	for i := 0; i < k; i++ { // a delivered data shard the compared shards prove corrupt: restored
		if fixRows[i] != nil && counts[i] != 0 {
			a, b := s.span(i)
			for x := range s.out[a:b] {
				s.out[a+int64(x)] ^= fixRows[i][x]
			}
		}
	}
	if rc == C.RS_E_CORRUPT {
		return s.out, ErrShardCorrupted
	}
	return s.out, nil
}

// Close frees the session.
func (s *DecodeSession) Close() {
	if s.h != nil {
		C.rs_session_close(s.h)
		s.h = nil
	}
}

// ---- encode sessions (DESIGN.md §5.18) --------------------------------------------------------

// EncodeSession is a progressive encode of one object whose parity rows stay on the device
// (rs_encode_session_open): Write (or Feed) each piece of the request body as it is read, then
// Finish for the n shards Encode would return. The body is kept, in Split's layout, in one
// buffer of n*S bytes whose tail receives the parity, so Finish copies nothing but the parity.
// On a profile or a machine the GPU codec does not serve it buffers the body and encodes at
// Finish. Like the rest of this package it has never been compiled where the library is
// developed. Not in the reference API.
type EncodeSession struct {
	c       *Codec
	h       *C.rs_encode_session
	profile ErasureProfile
	size    int64
	S       int
	mu      sync.Mutex
	buf     []byte // k*S body bytes, zero padded, then m*S parity bytes
	off     int64  // Write's running offset
}

// EncodeSession opens a session for a body of size bytes (the request's Content-Length).
func (c *Codec) EncodeSession(profile ErasureProfile, size int64) (*EncodeSession, error) {
	k, m := profile.DataShards, profile.ParityShards
	if k < 1 || m < 1 {
		return nil, ErrInvalidProfile
	}
	if size <= 0 {
		return nil, fmt.Errorf("erasure: failed to split data: %w", reedsolomon.ErrShortData)
	}
	S := int((size + int64(k) - 1) / int64(k))
	s := &EncodeSession{c: c, profile: profile, size: size, S: S, buf: make([]byte, (k+m)*S)}
	if k+m > 256 || m > 16 || size < int64(gpuMinBytes) || device() == nil {
		return s, nil
	}
	if rc := C.rs_encode_session_open(gpuCtx, C.int(k), C.int(m), C.size_t(size), &s.h); rc != C.RS_OK {
		return nil, fmt.Errorf("erasure: failed to create encoder: %w", upstreamErr(rc))
	}
	return s, nil
}

// Feed folds body bytes [off, off+len(data)) in, every byte exactly once, from any goroutine and
// in any order; it returns when data may be reused.
func (s *EncodeSession) Feed(off int64, data []byte) error {
	if off < 0 || len(data) == 0 || off+int64(len(data)) > s.size {
		return fmt.Errorf("erasure: body range [%d, %d) of %d", off, off+int64(len(data)), s.size)
	}
	if s.h != nil {
		var pin runtime.Pinner
		defer pin.Unpin()
		pin.Pin(&data[0])
		if rc := C.rs_encode_session_feed(s.h, C.uint64_t(off), (*C.uint8_t)(unsafe.Pointer(&data[0])), C.size_t(len(data))); rc != C.RS_OK {
			return fmt.Errorf("erasure: failed to encode parity: %w", upstreamErr(rc))
		}
	}
	s.mu.Lock()
	copy(s.buf[off:], data)
	s.mu.Unlock()
	return nil
}

// Write feeds p at the running offset: an io.Writer for io.Copy from the request body.
func (s *EncodeSession) Write(p []byte) (int, error) {
	if len(p) == 0 {
		return 0, nil
	}
	if err := s.Feed(s.off, p); err != nil {
		return 0, err
	}
	s.off += int64(len(p))
	return len(p), nil
}

// Finish returns the n shards, bit for bit Encode's for the body. Before the whole body has been
// fed it is ErrShortData and the session stays usable.
func (s *EncodeSession) Finish() ([][]byte, error) {
	k, m := s.profile.DataShards, s.profile.ParityShards
	if s.h == nil {
		s.mu.Lock()
		defer s.mu.Unlock()
		if s.off != s.size {
			return nil, fmt.Errorf("erasure: failed to split data: %w", reedsolomon.ErrShortData)
		}
		return s.c.cpuEncode(s.buf[:s.size], s.profile)
	}
	ptrs := newCArray(m)
	defer ptrs.free()
	var pin runtime.Pinner
	defer pin.Unpin()
	shards := make([][]byte, k+m)
	for i := range shards {
		shards[i] = s.buf[i*s.S : (i+1)*s.S : (i+1)*s.S]
		if i >= k {
			pin.Pin(&shards[i][0])
			ptrs.set(i-k, unsafe.Pointer(&shards[i][0]))
		}
	}
	var ss C.size_t
	if rc := C.rs_encode_session_finish(s.h, ptrs.at(0), &ss); rc != C.RS_OK {
		return nil, fmt.Errorf("erasure: failed to encode parity: %w", upstreamErr(rc))
	}
	return shards, nil
}

// Close frees the session.
func (s *EncodeSession) Close() {
	if s.h != nil {
		C.rs_encode_session_close(s.h)
		s.h = nil
	}
}

// Overwrite replaces bytes [offset, offset+len(data)) of the object whose n shards these are
// (Encode's layout: object byte x in data shard x/S at column x%S) and brings the parity up to
// date (rs_codec_overwrite): only the affected parity columns are read and rewritten, through
// one update batch of at most three column intervals, then data is copied into the data
// shards. Afterwards shards equal Encode of the overwritten object. The data shards the range
// does not touch may be nil. Not in the reference API.
func (c *Codec) Overwrite(shards [][]byte, profile ErasureProfile, offset int64, data []byte) error {
	k, m := profile.DataShards, profile.ParityShards
	if k < 1 || m < 1 {
		return ErrInvalidProfile
	}
	if k+m > 256 || device() == nil {
		return cpuOverwrite(shards, k, m, offset, data)
	}
	S, err := checkOverwrite(shards, k, m, offset, data)
	if err != nil {
		return err
	}
	ptrs := newCArray(k + m)
	defer ptrs.free()
	var pin runtime.Pinner
	defer pin.Unpin()
	for i, s := range shards {
		if len(s) == S {
			pin.Pin(&s[0])
			ptrs.set(i, unsafe.Pointer(&s[0]))
		}
	}
	pin.Pin(&data[0])
	return updateErr(C.rs_codec_overwrite(gpuCtx, C.int(k), C.int(m), C.size_t(S), ptrs.at(0),
		C.int64_t(offset), (*C.uint8_t)(unsafe.Pointer(&data[0])), C.size_t(len(data))))
}

// Correct repairs one object's present shards in place from the parity syndromes (rs_correct,
// DESIGN.md §5.13): in every byte column in which exactly one examined shard is corrupt, that
// byte is restored, however many shards the damage is spread over -- as long as the object
// compares three or more shards (present shards beyond the first k). counts[i] is the number
// of bytes of shard i that were changed, counts[k+m] the columns that still mismatch (more than
// one error in the column, or fewer than three compared shards: nothing is written there).
// Missing shards (nil or empty) are neither read nor rebuilt. Shards with a nonzero count are
// the ones to store back.
func (c *Codec) Correct(shards [][]byte, profile ErasureProfile) ([]uint64, error) {
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
	rc := C.rs_correct(gpuCtx, C.int(k), C.int(m), ptrs.at(0), &lens[0], &counts[0])
	if rc != C.RS_OK && rc != C.RS_E_CORRUPT { // RS_E_CORRUPT: counts[k+m] says how much is left
		return nil, decodeErr(rc)
	}
	out := make([]uint64, n+1)
	for i := range out {
		out[i] = uint64(counts[i])
	}
	return out, nil
}

// CorrectBatch is Correct for many objects of any sizes and erasures in one call
// (rs_correct_batch): a scrub over objs[b] = the n shards of object b as stored. counts[b] is
// Correct's; errs[b] is nil when nothing mismatched or every mismatching column was corrected,
// ErrShardCorrupted when a column is left (bytes already corrected stay corrected), and the
// object's own error otherwise. Only shards with corrected bytes are copied back from the
// device. On builds or hosts without the GPU codec every object reports ErrLocateUnavailable.
func (c *Codec) CorrectBatch(objs [][][]byte, profile ErasureProfile) (counts [][]uint64, errs []error) {
	k, m := profile.DataShards, profile.ParityShards
	errs = make([]error, len(objs))
	counts = make([][]uint64, len(objs))
	fail := func(err error) ([][]uint64, []error) {
		for b := range errs {
			if errs[b] == nil {
				errs[b] = err
			}
		}
		return counts, errs
	}
	if k < 1 || m < 1 {
		return fail(ErrInvalidProfile)
	}
	n := k + m
	if len(objs) == 0 {
		return counts, errs
	}
	if n > 256 || device() == nil {
		return fail(ErrLocateUnavailable)
	}
	ptrs := newCArray(len(objs) * n)
	defer ptrs.free()
	lens := make([]C.size_t, len(objs)*n)
	cn := make([]C.uint64_t, len(objs)*(n+1))
	status := make([]C.int, len(objs))
	var pin runtime.Pinner
	defer pin.Unpin()
	for b, shards := range objs {
		if len(shards) != n {
			errs[b] = fmt.Errorf("erasure: reconstruction failed: %w", reedsolomon.ErrTooFewShards)
			continue // all lens 0 and no pointers: the stripe reports RS_E_NO_DATA, ignored
		}
		pinShards(&pin, ptrs, lens, b*n, shards)
	}
	rc := C.rs_correct_batch(gpuCtx, C.int(k), C.int(m), C.int(len(objs)), ptrs.at(0), &lens[0],
		&cn[0], &status[0])
	if rc != C.RS_OK && !hasStatus(status, rc) { // a call-level error
		return fail(decodeErr(rc))
	}
	for b := range objs {
		if errs[b] != nil {
			continue
		}
		counts[b] = make([]uint64, n+1)
		for i := range counts[b] {
			counts[b][i] = uint64(cn[b*(n+1)+i])
		}
		errs[b] = decodeErr(status[b])
	}
	return counts, errs
}

// DecodeCorrect is Decode after one Correct over the present shards
// (rs_codec_decode_correct): an object whose fetched shards hold scattered bad sectors -- one
// corrupt byte per column, on any number of shards -- is served where Decode and DecodeHeal end
// in ErrShardCorrupted. It returns the object and the indices of the shards that had bytes
// corrected in `shards`, for the caller to store back; it fails with ErrShardCorrupted exactly
// when Decode still does after the correction. Every other error, the join and the trim are
// Decode's. Objects the GPU does not take are decoded by the CPU codec, which corrects nothing.
func (c *Codec) DecodeCorrect(shards [][]byte, profile ErasureProfile, originalSize int64) ([]byte, []int, error) {
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
		lens[i] = C.size_t(len(bufs[i]))
		if len(bufs[i]) == 0 && S > 0 { // upstream Reconstruct allocates missing shards
			if cap(bufs[i]) >= S {
				bufs[i] = bufs[i][:S]
			} else {
				bufs[i] = make([]byte, S)
			}
		}
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
	rc := C.rs_codec_decode_correct(gpuCtx, C.int(k), C.int(m), ptrs.at(0), &lens[0], out,
		C.int64_t(originalSize), &flags[0])
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
	var corrected []int
	for i := range flags {
		if flags[i] != 0 {
			corrected = append(corrected, i)
		}
	}
	return buf, corrected, nil
}
