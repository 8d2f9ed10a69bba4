package erasure

// The checksummed batches on the CPU: what EncodeBatchSums / DecodeBatchSums compute on a
// build without the GPU codec (codec_cpu_sums.go) and what the GPU build falls back to where
// no device can run them (codec_rocm_sums.go). They loop over cpuEncode / cpuDecode and
// ShardChecksum, as Manager.StoreFile and Manager.RetrieveFile do per object.

func cpuEncodeBatchSums(c *Codec, objs [][]byte, profile ErasureProfile) ([][][]byte, [][]string, []error) {
	out := make([][][]byte, len(objs))
	sums := make([][]string, len(objs))
	errs := make([]error, len(objs))
	for b, d := range objs {
		out[b], errs[b] = c.cpuEncode(d, profile)
		if errs[b] != nil {
			continue
		}
		sums[b] = make([]string, len(out[b]))
		for i, s := range out[b] {
			sums[b][i] = ShardChecksum(s)
		}
	}
	return out, sums, errs
}

// A present shard whose checksum differs is dropped before the decode (manager.go:283-296);
// upstream Reconstruct then allocates it anew, and the caller's slice header is pointed at the
// rebuilt shard like those of the missing ones.
func cpuDecodeBatchSums(c *Codec, shards [][][]byte, sums [][]string, profile ErasureProfile, sizes []int64) ([][]byte, [][]int, []error) {
	out := make([][]byte, len(shards))
	bad := make([][]int, len(shards))
	errs := make([]error, len(shards))
	for b, sh := range shards {
		work := make([][]byte, len(sh))
		copy(work, sh)
		for i, s := range sh {
			if len(s) > 0 && len(sums[b]) == len(sh) && ShardChecksum(s) != sums[b][i] {
				bad[b] = append(bad[b], i)
				work[i] = nil
			}
		}
		out[b], errs[b] = c.cpuDecode(work, profile, sizes[b])
		for i := range sh {
			if len(work[i]) != 0 { // filled by Reconstruct, or untouched
				sh[i] = work[i]
			}
		}
	}
	return out, bad, errs
}
