package erasure

import (
	"fmt"

	"github.com/klauspost/reedsolomon"
)

// The CPU forms of the calls that update parity in place (UpdateParity, EncodeIdx, UpdateBatch,
// Overwrite) and of the progressive decode (DecodeIdx, DecodeIdxBatch, DecodeCheck,
// DecodeCheckBatch): upstream Update / EncodeIdx / DecodeIdx. Both builds use them: the default build for every
// call, the GPU build for k+m > 256 and when there is no device.

// cpuUpdateParity is upstream enc.Update(shards, newData): shards holds the old data shards
// (only the changed ones are read) and the m parity shards, updated in place; newData has k
// entries, nil = unchanged. The data entries of shards stay as they are.
func cpuUpdateParity(shards, newData [][]byte, k, m int) error {
	enc, err := reedsolomon.New(k, m)
	if err != nil {
		return fmt.Errorf("erasure: failed to create encoder: %w", err)
	}
	if err := enc.Update(shards, newData); err != nil {
		return fmt.Errorf("erasure: failed to update parity: %w", err)
	}
	return nil
}

// cpuEncodeIdx is upstream enc.EncodeIdx(dataShard, idx, parity).
func cpuEncodeIdx(dataShard []byte, idx int, parity [][]byte, k, m int) error {
	enc, err := reedsolomon.New(k, m)
	if err != nil {
		return fmt.Errorf("erasure: failed to create encoder: %w", err)
	}
	if err := enc.EncodeIdx(dataShard, idx, parity); err != nil {
		return fmt.Errorf("erasure: failed to update parity: %w", err)
	}
	return nil
}

// cpuDecodeIdx is upstream enc.DecodeIdx(dst, expectInput, input): the contribution of the
// delivered input shards is added into the wanted dst shards.
func cpuDecodeIdx(dst [][]byte, expectInput []bool, input [][]byte, k, m int) error {
	enc, err := reedsolomon.New(k, m)
	if err != nil {
		return fmt.Errorf("erasure: failed to create encoder: %w", err)
	}
	if err := enc.DecodeIdx(dst, expectInput, input); err != nil {
		return fmt.Errorf("erasure: failed to decode: %w", err)
	}
	return nil
}

// cpuDecodeCheck is DecodeCheck on the CPU (DESIGN.md §5.15): upstream DecodeIdx into the wanted
// shards and the accumulators alike, the compared shards that arrive with the call XORed into
// their accumulators, and in a final call the result tested for zero on copies, so that no
// accumulator is written.
func cpuDecodeCheck(dst, check [][]byte, expectInput []bool, input [][]byte, final bool, k, m int) error {
	wrap := func(err error) error { return fmt.Errorf("erasure: failed to decode: %w", err) }
	n := k + m
	if len(dst) != n || len(check) != n || len(expectInput) != n || len(input) != n {
		return wrap(reedsolomon.ErrTooFewShards)
	}
	rows, in := make([][]byte, n), make([][]byte, n)
	fed := false
	for i := 0; i < n; i++ {
		rows[i] = dst[i]
		if len(check[i]) > 0 {
			if expectInput[i] || len(dst[i]) > 0 {
				return wrap(reedsolomon.ErrInvalidInput)
			}
			rows[i] = check[i]
			if final {
				rows[i] = append([]byte(nil), check[i]...)
			}
		}
		if len(input[i]) > 0 && !expectInput[i] {
			if len(check[i]) == 0 {
				return wrap(reedsolomon.ErrInvalidInput)
			}
			continue // the compared shard itself: XORed in below
		}
		in[i] = input[i]
		fed = fed || len(input[i]) > 0
	}
	if fed {
		if err := cpuDecodeIdx(rows, expectInput, in, k, m); err != nil {
			return err
		}
	}
	corrupt := false
	for i := 0; i < n; i++ {
		if len(check[i]) == 0 {
			continue
		}
		if len(input[i]) > 0 {
			if len(input[i]) != len(rows[i]) {
				return wrap(reedsolomon.ErrShardSize)
			}
			for x, b := range input[i] {
				rows[i][x] ^= b
			}
		}
		for _, b := range rows[i] {
			corrupt = corrupt || (final && b != 0)
		}
	}
	if corrupt {
		return ErrShardCorrupted
	}
	return nil
}

// cpuDecodeRepair is DecodeRepair on the CPU (DESIGN.md §5.16). The CPU codec has no locator
// (the reference finds a bad shard by its checksum), so this form never repairs: it is the final
// DecodeCheck, with every mismatching byte column counted as unexplained in counts[k+m], no fix
// buffer touched, and ErrShardCorrupted where a column mismatches -- what the GPU form reports
// for a stripe with fewer than three compared shards. A fix buffer at an index that is neither
// expected nor compared is refused as the library refuses it.
func cpuDecodeRepair(dst, check, fix [][]byte, expectInput []bool, input [][]byte, k, m int) ([]uint64, error) {
	n := k + m
	if len(fix) != n || len(check) != n || len(expectInput) != n {
		return nil, fmt.Errorf("erasure: failed to decode: %w", reedsolomon.ErrTooFewShards)
	}
	rows := 0
	for i := 0; i < n; i++ {
		if len(fix[i]) > 0 && !expectInput[i] && len(check[i]) == 0 {
			return nil, fmt.Errorf("erasure: failed to decode: %w", reedsolomon.ErrInvalidInput)
		}
		if i < len(dst) && (len(dst[i]) > 0 || len(check[i]) > 0) {
			rows++
		}
	}
	if rows > 16 {
		return nil, fmt.Errorf("erasure: failed to decode: %d wanted and compared shards, at most 16", rows)
	}
	// the syndromes on copies: a final call writes no accumulator
	acc := make([][]byte, n)
	for i := range check {
		if len(check[i]) > 0 {
			acc[i] = append([]byte(nil), check[i]...)
		}
	}
	if err := cpuDecodeCheck(dst, acc, expectInput, input, false, k, m); err != nil {
		return nil, err
	}
	counts := make([]uint64, n+1)
	S := 0
	for i := range acc {
		if len(acc[i]) > S {
			S = len(acc[i])
		}
	}
	for x := 0; x < S; x++ {
		for i := range acc {
			if x < len(acc[i]) && acc[i][x] != 0 {
				counts[n]++
				break
			}
		}
	}
	if counts[n] != 0 {
		return counts, ErrShardCorrupted
	}
	return counts, nil
}

// overwriteStripes cuts an overwrite of object bytes [offset, offset+len(data)) into at most
// three stripes over disjoint column intervals of the S-byte shards (csrc/overwrite_plan.hpp):
// the range's first shard changes from its first column on, its last shard up to its last
// column, the shards between them everywhere. Stripe j is (old[j], new[j], parity[j]): subslices
// of the shards and of data, the n-entry and k-entry forms upstream Update takes.
func overwriteStripes(shards [][]byte, k, m, S int, offset int64, data []byte) (old, nw [][][]byte) {
	off, end := int(offset), int(offset)+len(data)
	a, z := off/S, (end-1)/S
	ca, cz := off%S, (end-1)%S+1
	cuts := []int{0, ca, cz, S}
	if a == z {
		cuts = []int{ca, cz}
	} else if ca > cz {
		cuts = []int{0, cz, ca, S}
	}
	for q := 0; q+1 < len(cuts); q++ {
		lo, hi := cuts[q], cuts[q+1]
		if lo >= hi {
			continue
		}
		s0, s1 := a, z
		if a != z && lo < ca {
			s0 = a + 1
		}
		if a != z && hi > cz {
			s1 = z - 1
		}
		if s0 > s1 {
			continue
		}
		o := make([][]byte, k+m)
		w := make([][]byte, k)
		for i := s0; i <= s1; i++ {
			o[i] = shards[i][lo:hi]
			w[i] = data[i*S+lo-off : i*S+hi-off]
		}
		for j := k; j < k+m; j++ {
			o[j] = shards[j][lo:hi]
		}
		old = append(old, o)
		nw = append(nw, w)
	}
	return old, nw
}

// checkOverwrite validates Overwrite's arguments and returns the shard size.
func checkOverwrite(shards [][]byte, k, m int, offset int64, data []byte) (int, error) {
	if k < 1 || m < 1 {
		return 0, ErrInvalidProfile
	}
	if len(shards) != k+m {
		return 0, fmt.Errorf("erasure: failed to update parity: %w", reedsolomon.ErrTooFewShards)
	}
	S := 0
	for _, s := range shards {
		if len(s) > 0 {
			S = len(s)
			break
		}
	}
	if S == 0 || len(data) == 0 || offset < 0 || offset+int64(len(data)) > int64(k)*int64(S) {
		return 0, fmt.Errorf("erasure: overwrite of bytes [%d, %d) outside the object's %d shard bytes",
			offset, offset+int64(len(data)), int64(k)*int64(S))
	}
	first, last := int(offset)/S, (int(offset)+len(data)-1)/S
	for i := range shards {
		if (i >= first && i <= last) || i >= k {
			if len(shards[i]) != S {
				return 0, fmt.Errorf("erasure: failed to update parity: %w", reedsolomon.ErrShardSize)
			}
		}
	}
	return S, nil
}

// copyIntoShards writes data over object bytes [offset, offset+len(data)) of the data shards.
func copyIntoShards(shards [][]byte, S int, offset int64, data []byte) {
	off := int(offset)
	for len(data) > 0 {
		i, c := off/S, off%S
		n := copy(shards[i][c:], data)
		data = data[n:]
		off += n
	}
}

// cpuOverwrite is Overwrite on the CPU codec: upstream Update per column interval, then the
// data bytes.
func cpuOverwrite(shards [][]byte, k, m int, offset int64, data []byte) error {
	S, err := checkOverwrite(shards, k, m, offset, data)
	if err != nil {
		return err
	}
	old, nw := overwriteStripes(shards, k, m, S, offset, data)
	for j := range old {
		if err := cpuUpdateParity(old[j], nw[j], k, m); err != nil {
			return err
		}
	}
	copyIntoShards(shards, S, offset, data)
	return nil
}
