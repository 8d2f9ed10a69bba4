package erasure

import (
	"fmt"

	"github.com/klauspost/reedsolomon"
)

// The CPU forms of the calls that rebuild only the shards a caller asks for (DecodeData,
// DecodeDataBatch, RepairSome): upstream ReconstructData / ReconstructSome. Both builds use
// them: the default build for every call, the GPU build for k+m > 256, for objects below the
// GPU threshold and when there is no device.

// verifyPresent checks the present shards of a stripe whose wanted shards have been rebuilt.
// Upstream Verify needs every shard, so the nil entries are completed in a private copy and
// the caller's slice keeps them nil.
func verifyPresent(enc reedsolomon.Encoder, shards [][]byte) error {
	all := make([][]byte, len(shards))
	copy(all, shards)
	for _, s := range all {
		if len(s) == 0 {
			if err := enc.Reconstruct(all); err != nil {
				return fmt.Errorf("erasure: reconstruction failed: %w", err)
			}
			break
		}
	}
	ok, err := enc.Verify(all)
	if err != nil {
		return fmt.Errorf("erasure: verification failed: %w", err)
	}
	if !ok {
		return ErrShardCorrupted
	}
	return nil
}

// cpuDecodeData is the reference Decode with ReconstructData in Reconstruct's place: missing
// parity entries stay nil.
func cpuDecodeData(shards [][]byte, profile ErasureProfile, originalSize int64) ([]byte, error) {
	k, m := profile.DataShards, profile.ParityShards
	if k < 1 || m < 1 {
		return nil, ErrInvalidProfile
	}
	enc, err := reedsolomon.New(k, m)
	if err != nil {
		return nil, fmt.Errorf("erasure: failed to create decoder: %w", err)
	}
	if err := enc.ReconstructData(shards); err != nil {
		return nil, fmt.Errorf("erasure: reconstruction failed: %w", err)
	}
	if err := verifyPresent(enc, shards); err != nil {
		return nil, err
	}
	buf := make([]byte, 0, originalSize)
	for i := 0; i < k; i++ {
		buf = append(buf, shards[i]...)
	}
	if int64(len(buf)) < originalSize {
		return nil, ErrInsufficientShards
	}
	return buf[:originalSize], nil
}

// cpuRepairSome is RepairSome's per-object CPU form: upstream ReconstructSome + Verify of the
// present shards. want has n flags.
func cpuRepairSome(shards [][]byte, want []bool, k, m int) error {
	if want == nil {
		want = make([]bool, k+m)
		for i := range want {
			want[i] = true
		}
	}
	enc, err := reedsolomon.New(k, m)
	if err != nil {
		return fmt.Errorf("erasure: failed to create decoder: %w", err)
	}
	if err := enc.ReconstructSome(shards, want); err != nil {
		return fmt.Errorf("erasure: reconstruction failed: %w", err)
	}
	return verifyPresent(enc, shards)
}
