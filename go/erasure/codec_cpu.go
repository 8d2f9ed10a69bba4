//go:build !(rocm && cgo)

package erasure

import (
	"errors"
	"fmt"
	"sync"
)

// Builds without the GPU codec (the default CGO_ENABLED=0 release builds,
// Dockerfile:20-22, builds.sh:8-20) keep the reference codec: after codec.go.diff its
// methods are named cpuEncode / cpuDecode, and these two forward to them, so the binary
// behaves exactly as before.

// Encode splits data into DataShards pieces and computes ParityShards parity shards.
func (c *Codec) Encode(data []byte, profile ErasureProfile) ([][]byte, error) {
	return c.cpuEncode(data, profile)
}

// Decode reconstructs the original data from shards (nil entries are missing).
func (c *Codec) Decode(shards [][]byte, profile ErasureProfile, originalSize int64) ([]byte, error) {
	return c.cpuDecode(shards, profile, originalSize)
}

// EncodeBatch is Encode per object on builds without the GPU codec (the GPU build runs the
// whole batch as one call, codec_rocm.go).
func (c *Codec) EncodeBatch(objs [][]byte, profile ErasureProfile) ([][][]byte, []error) {
	out := make([][][]byte, len(objs))
	errs := make([]error, len(objs))
	for b, d := range objs {
		out[b], errs[b] = c.cpuEncode(d, profile)
	}
	return out, errs
}

// DecodeBatch is Decode per object on builds without the GPU codec. sizes holds one
// original size per object.
func (c *Codec) DecodeBatch(shards [][][]byte, profile ErasureProfile, sizes []int64) ([][]byte, []error) {
	out := make([][]byte, len(shards))
	errs := make([]error, len(shards))
	for b := range shards {
		if len(sizes) != len(shards) {
			errs[b] = fmt.Errorf("erasure: %d sizes for %d objects", len(sizes), len(shards))
			continue
		}
		out[b], errs[b] = c.cpuDecode(shards[b], profile, sizes[b])
	}
	return out, errs
}

// DecodeData is Decode with upstream ReconstructData in Reconstruct's place: missing data
// shards are rebuilt and joined, missing parity shards stay nil (the GPU build runs
// rs_codec_decode_data, codec_rocm.go).
func (c *Codec) DecodeData(shards [][]byte, profile ErasureProfile, originalSize int64) ([]byte, error) {
	return cpuDecodeData(shards, profile, originalSize)
}

// DecodeDataBatch is DecodeData per object on builds without the GPU codec.
func (c *Codec) DecodeDataBatch(shards [][][]byte, profile ErasureProfile, sizes []int64) ([][]byte, []error) {
	out := make([][]byte, len(shards))
	errs := make([]error, len(shards))
	for b := range shards {
		if len(sizes) != len(shards) {
			errs[b] = fmt.Errorf("erasure: %d sizes for %d objects", len(sizes), len(shards))
			continue
		}
		out[b], errs[b] = cpuDecodeData(shards[b], profile, sizes[b])
	}
	return out, errs
}

// RepairSome is upstream ReconstructSome per object on builds without the GPU codec:
// want[b] (nil: every missing shard) names the entries of objs[b] to rebuild.
func (c *Codec) RepairSome(objs [][][]byte, want [][]bool, profile ErasureProfile) []error {
	errs := make([]error, len(objs))
	for b, shards := range objs {
		var w []bool
		if want != nil {
			w = want[b]
		}
		errs[b] = cpuRepairSome(shards, w, profile.DataShards, profile.ParityShards)
	}
	return errs
}

// The pinned-buffer helpers of the GPU build (codec_rocm.go) exist here too, so callers
// compile on every build: there is no device, so HostBuffer and BodyBuffer return nil
// (read into heap buffers as before), FreeHostBuffer ignores its argument and DecodePinned
// is Decode.

// HostBuffer returns nil on builds without the GPU codec.
func HostBuffer(n int) []byte { return nil }

// BodyBuffer returns nil on builds without the GPU codec.
func BodyBuffer(size int, profile ErasureProfile) []byte { return nil }

// FreeHostBuffer does nothing on builds without the GPU codec.
func FreeHostBuffer(b []byte) {}

// DecodePinned is Decode on builds without the GPU codec.
func (c *Codec) DecodePinned(shards [][]byte, profile ErasureProfile, originalSize int64) ([]byte, error) {
	return c.cpuDecode(shards, profile, originalSize)
}

// UpdateParity is upstream enc.Update(shards, newData) on builds without the GPU codec: the m
// parity entries of shards are updated in place from the old (shards) and new (newData, nil =
// unchanged) bytes of the changed data shards.
func (c *Codec) UpdateParity(shards, newData [][]byte, profile ErasureProfile) error {
	if profile.DataShards < 1 || profile.ParityShards < 1 {
		return ErrInvalidProfile
	}
	return cpuUpdateParity(shards, newData, profile.DataShards, profile.ParityShards)
}

// EncodeIdx is upstream enc.EncodeIdx(dataShard, idx, parity) on builds without the GPU codec.
func (c *Codec) EncodeIdx(dataShard []byte, idx int, parity [][]byte, profile ErasureProfile) error {
	if profile.DataShards < 1 || profile.ParityShards < 1 {
		return ErrInvalidProfile
	}
	return cpuEncodeIdx(dataShard, idx, parity, profile.DataShards, profile.ParityShards)
}

// UpdateBatch is UpdateParity per stripe on builds without the GPU codec.
func (c *Codec) UpdateBatch(shards, newData [][][]byte, profile ErasureProfile) []error {
	errs := make([]error, len(shards))
	for b := range shards {
		if len(newData) != len(shards) {
			errs[b] = fmt.Errorf("erasure: %d new-data rows for %d stripes", len(newData), len(shards))
			continue
		}
		errs[b] = c.UpdateParity(shards[b], newData[b], profile)
	}
	return errs
}

// DecodeIdx is upstream enc.DecodeIdx(dst, expectInput, input) on builds without the GPU codec.
func (c *Codec) DecodeIdx(dst [][]byte, expectInput []bool, input [][]byte, profile ErasureProfile) error {
	if profile.DataShards < 1 || profile.ParityShards < 1 {
		return ErrInvalidProfile
	}
	return cpuDecodeIdx(dst, expectInput, input, profile.DataShards, profile.ParityShards)
}

// DecodeIdxBatch is DecodeIdx per stripe on builds without the GPU codec.
func (c *Codec) DecodeIdxBatch(dst [][][]byte, expectInput [][]bool, input [][][]byte, profile ErasureProfile) []error {
	errs := make([]error, len(dst))
	for b := range dst {
		if len(expectInput) != len(dst) || len(input) != len(dst) {
			errs[b] = fmt.Errorf("erasure: %d expect rows and %d input rows for %d stripes", len(expectInput),
				len(input), len(dst))
			continue
		}
		errs[b] = c.DecodeIdx(dst[b], expectInput[b], input[b], profile)
	}
	return errs
}

// DecodeCheck is DecodeIdx with compared shards (DESIGN.md §5.15) on builds without the GPU
// codec.
func (c *Codec) DecodeCheck(dst, check [][]byte, expectInput []bool, input [][]byte, final bool, profile ErasureProfile) error {
	if profile.DataShards < 1 || profile.ParityShards < 1 {
		return ErrInvalidProfile
	}
	return cpuDecodeCheck(dst, check, expectInput, input, final, profile.DataShards, profile.ParityShards)
}

// DecodeCheckBatch is DecodeCheck per stripe on builds without the GPU codec.
func (c *Codec) DecodeCheckBatch(dst, check [][][]byte, expectInput [][]bool, input [][][]byte, final bool, profile ErasureProfile) []error {
	errs := make([]error, len(dst))
	for b := range dst {
		if len(check) != len(dst) || len(expectInput) != len(dst) || len(input) != len(dst) {
			errs[b] = fmt.Errorf("erasure: %d check rows, %d expect rows and %d input rows for %d stripes", len(check),
				len(expectInput), len(input), len(dst))
			continue
		}
		errs[b] = c.DecodeCheck(dst[b], check[b], expectInput[b], input[b], final, profile)
	}
	return errs
}

// DecodeRepair is the final DecodeCheck with fix buffers (DESIGN.md §5.16) on builds without the
// GPU codec: cpuDecodeRepair, which flags and counts and never repairs.
func (c *Codec) DecodeRepair(dst, check, fix [][]byte, expectInput []bool, input [][]byte, profile ErasureProfile) ([]uint64, error) {
	if profile.DataShards < 1 || profile.ParityShards < 1 {
		return nil, ErrInvalidProfile
	}
	return cpuDecodeRepair(dst, check, fix, expectInput, input, profile.DataShards, profile.ParityShards)
}

// DecodeRepairBatch is DecodeRepair per stripe on builds without the GPU codec.
func (c *Codec) DecodeRepairBatch(dst, check, fix [][][]byte, expectInput [][]bool, input [][][]byte, profile ErasureProfile) ([][]uint64, []error) {
	errs := make([]error, len(dst))
	counts := make([][]uint64, len(dst))
	for b := range dst {
		if len(check) != len(dst) || len(fix) != len(dst) || len(expectInput) != len(dst) || len(input) != len(dst) {
			errs[b] = fmt.Errorf("erasure: %d check rows, %d fix rows, %d expect rows and %d input rows for %d stripes",
				len(check), len(fix), len(expectInput), len(input), len(dst))
			continue
		}
		counts[b], errs[b] = c.DecodeRepair(dst[b], check[b], fix[b], expectInput[b], input[b], profile)
	}
	return counts, errs
}

// DecodeSession (DESIGN.md §5.17) on builds without the GPU codec: it collects the shards as
// they are fed and decodes them at Finish.
type DecodeSession struct {
	c       *Codec
	profile ErasureProfile
	size    int64
	mu      sync.Mutex
	fed     [][]byte
}

// DecodeSession opens a session; expect, compare and repair are the GPU codec's to use.
func (c *Codec) DecodeSession(profile ErasureProfile, originalSize int64, expect, compare []int, repair bool) (*DecodeSession, error) {
	if profile.DataShards < 1 || profile.ParityShards < 1 {
		return nil, ErrInvalidProfile
	}
	return &DecodeSession{c: c, profile: profile, size: originalSize,
		fed: make([][]byte, profile.DataShards+profile.ParityShards)}, nil
}

// Feed keeps a copy of shard idx.
func (s *DecodeSession) Feed(idx int, shard []byte) error {
	if idx < 0 || idx >= len(s.fed) {
		return fmt.Errorf("erasure: shard index %d of %d", idx, len(s.fed))
	}
	s.mu.Lock()
	defer s.mu.Unlock()
	s.fed[idx] = append([]byte(nil), shard...)
	return nil
}

// Finish is Decode of the shards fed so far.
func (s *DecodeSession) Finish() ([]byte, error) {
	s.mu.Lock()
	defer s.mu.Unlock()
	return s.c.Decode(s.fed, s.profile, s.size)
}

// Close frees nothing here.
func (s *DecodeSession) Close() {}

// EncodeSession (DESIGN.md §5.18) on builds without the GPU codec: it buffers the body as it is
// fed and encodes it at Finish.
type EncodeSession struct {
	c       *Codec
	profile ErasureProfile
	size    int64
	mu      sync.Mutex
	body    []byte
	fed     int64
	off     int64
}

// EncodeSession opens a session for a body of size bytes.
func (c *Codec) EncodeSession(profile ErasureProfile, size int64) (*EncodeSession, error) {
	if profile.DataShards < 1 || profile.ParityShards < 1 {
		return nil, ErrInvalidProfile
	}
	if size < 0 {
		size = 0
	}
	return &EncodeSession{c: c, profile: profile, size: size, body: make([]byte, size)}, nil
}

// Feed keeps body bytes [off, off+len(data)).
func (s *EncodeSession) Feed(off int64, data []byte) error {
	if off < 0 || off+int64(len(data)) > s.size {
		return fmt.Errorf("erasure: body range [%d, %d) of %d", off, off+int64(len(data)), s.size)
	}
	s.mu.Lock()
	defer s.mu.Unlock()
	copy(s.body[off:], data)
	s.fed += int64(len(data))
	return nil
}

// Write feeds p at the running offset.
func (s *EncodeSession) Write(p []byte) (int, error) {
	if err := s.Feed(s.off, p); err != nil {
		return 0, err
	}
	s.off += int64(len(p))
	return len(p), nil
}

// Finish is Encode of the buffered body.
func (s *EncodeSession) Finish() ([][]byte, error) {
	s.mu.Lock()
	defer s.mu.Unlock()
	return s.c.cpuEncode(s.body, s.profile)
}

// Close frees nothing here.
func (s *EncodeSession) Close() {}

// ErrLocateUnavailable is what Locate reports on builds without the GPU codec: the CPU codec
// has no locator (the reference finds a bad shard by its checksum, manager.go:250-320).
var ErrLocateUnavailable = errors.New("erasure: locating corrupt shards needs the GPU codec")

// Locate reports ErrLocateUnavailable on builds without the GPU codec.
func (c *Codec) Locate(shards [][]byte, profile ErasureProfile) ([]uint64, error) {
	if profile.DataShards < 1 || profile.ParityShards < 1 {
		return nil, ErrInvalidProfile
	}
	return nil, ErrLocateUnavailable
}

// HealBatch is RepairSome of every missing shard on builds without the GPU codec: nothing is
// healed, and an object whose present shards mismatch reports ErrShardCorrupted as before.
func (c *Codec) HealBatch(objs [][][]byte, profile ErasureProfile) ([][]int, []error) {
	return make([][]int, len(objs)), c.RepairSome(objs, nil, profile)
}

// DecodeHeal is Decode on builds without the GPU codec: nothing is healed.
func (c *Codec) DecodeHeal(shards [][]byte, profile ErasureProfile, originalSize int64) ([]byte, []int, error) {
	out, err := c.cpuDecode(shards, profile, originalSize)
	return out, nil, err
}

// ErrMaxErrors is what the ...Max calls report for maxErrors outside 1..2.
var ErrMaxErrors = errors.New("erasure: maxErrors must be 1 or 2")

// LocateMax, HealBatchMax and DecodeHealMax are Locate, HealBatch and DecodeHeal on builds
// without the GPU codec, whatever the maximum: nothing is located or healed.
func (c *Codec) LocateMax(shards [][]byte, profile ErasureProfile, maxErrors int) ([]uint64, error) {
	if maxErrors < 1 || maxErrors > 2 {
		return nil, ErrMaxErrors
	}
	return c.Locate(shards, profile)
}

func (c *Codec) HealBatchMax(objs [][][]byte, profile ErasureProfile, maxErrors int) ([][]int, []error) {
	if maxErrors < 1 || maxErrors > 2 {
		errs := make([]error, len(objs))
		for b := range errs {
			errs[b] = ErrMaxErrors
		}
		return make([][]int, len(objs)), errs
	}
	return c.HealBatch(objs, profile)
}

func (c *Codec) DecodeHealMax(shards [][]byte, profile ErasureProfile, originalSize int64, maxErrors int) ([]byte, []int, error) {
	if maxErrors < 1 || maxErrors > 2 {
		return nil, nil, ErrMaxErrors
	}
	return c.DecodeHeal(shards, profile, originalSize)
}

// Correct and CorrectBatch report ErrLocateUnavailable on builds without the GPU codec: the CPU
// codec has no syndrome decoder. Nothing is written.
func (c *Codec) Correct(shards [][]byte, profile ErasureProfile) ([]uint64, error) {
	if profile.DataShards < 1 || profile.ParityShards < 1 {
		return nil, ErrInvalidProfile
	}
	return nil, ErrLocateUnavailable
}

func (c *Codec) CorrectBatch(objs [][][]byte, profile ErasureProfile) ([][]uint64, []error) {
	errs := make([]error, len(objs))
	for b := range errs {
		errs[b] = ErrLocateUnavailable
		if profile.DataShards < 1 || profile.ParityShards < 1 {
			errs[b] = ErrInvalidProfile
		}
	}
	return make([][]uint64, len(objs)), errs
}

// DecodeCorrect is Decode on builds without the GPU codec: nothing is corrected.
func (c *Codec) DecodeCorrect(shards [][]byte, profile ErasureProfile, originalSize int64) ([]byte, []int, error) {
	out, err := c.cpuDecode(shards, profile, originalSize)
	return out, nil, err
}

// Overwrite replaces object bytes [offset, offset+len(data)) in the data shards and updates
// the affected parity columns with upstream Update, on builds without the GPU codec.
func (c *Codec) Overwrite(shards [][]byte, profile ErasureProfile, offset int64, data []byte) error {
	return cpuOverwrite(shards, profile.DataShards, profile.ParityShards, offset, data)
}
