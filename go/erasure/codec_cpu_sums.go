//go:build !(rocm && cgo)

package erasure

import "fmt"

// EncodeBatchSums is EncodeBatch plus every shard's ShardChecksum on builds without the GPU
// codec (the GPU build takes the checksums on the way through its pipeline,
// codec_rocm_sums.go).
func (c *Codec) EncodeBatchSums(objs [][]byte, profile ErasureProfile) ([][][]byte, [][]string, []error) {
	return cpuEncodeBatchSums(c, objs, profile)
}

// DecodeBatchSums is DecodeBatch behind the retrieve side's checksum pass on builds without
// the GPU codec: a present shard whose ShardChecksum differs from sums[b][i] is dropped,
// listed in bad[b] and rebuilt.
func (c *Codec) DecodeBatchSums(shards [][][]byte, sums [][]string, profile ErasureProfile, sizes []int64) ([][]byte, [][]int, []error) {
	if len(sizes) != len(shards) || len(sums) != len(shards) {
		errs := make([]error, len(shards))
		for b := range errs {
			errs[b] = fmt.Errorf("erasure: %d sizes and %d checksum lists for %d objects", len(sizes), len(sums), len(shards))
		}
		return make([][]byte, len(shards)), make([][]int, len(shards)), errs
	}
	return cpuDecodeBatchSums(c, shards, sums, profile, sizes)
}
