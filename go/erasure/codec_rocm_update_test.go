//go:build rocm && cgo

package erasure

// UpdateParity, EncodeIdx, UpdateBatch and Overwrite against upstream Update / EncodeIdx /
// Encode: parity bytes, untouched data shards, and the errors.
// Needs a HIP device: `go test -tags rocm ./erasure/` on a GPU box. Never compiled where the
// library is developed (no Go toolchain there): treat a first run's failures as the test's.

import (
	"bytes"
	"errors"
	"testing"

	"github.com/klauspost/reedsolomon"
)

// changedCopy returns newData (k entries, nil = unchanged) that differs from full in the
// shards of `changed`, and the shards an Encode of the new data gives.
func changedCopy(t *testing.T, c *Codec, full [][]byte, p ErasureProfile, changed []int, seed int) ([][]byte, [][]byte) {
	k := p.DataShards
	S := len(full[0])
	newData := make([][]byte, k)
	want := cloneShards(full)
	for _, i := range changed {
		nd := randBytes(int64(seed+i), S)
		nd[0] = full[i][0] ^ 0x80
		newData[i] = nd
		want[i] = nd
	}
	enc, err := reedsolomon.New(k, p.ParityShards)
	if err != nil {
		t.Fatal(err)
	}
	if err := enc.Encode(want); err != nil {
		t.Fatal(err)
	}
	return newData, want
}

func TestGPUUpdateParityMatchesUpstream(t *testing.T) {
	withGPU(t)
	c := NewCodec()
	for _, p := range []ErasureProfile{{DataShards: 4, ParityShards: 2}, {DataShards: 10, ParityShards: 4}, {DataShards: 10, ParityShards: 20}} {
		k, m := p.DataShards, p.ParityShards
		for _, size := range []int{k, 17 * k, 1 << 20, 3<<20 + 17} {
			full, err := c.cpuEncode(randBytes(int64(size), size), p)
			if err != nil {
				t.Fatal(err)
			}
			for _, changed := range [][]int{{0}, {k - 1}, {1, 2}, {}} {
				newData, want := changedCopy(t, c, full, p, changed, size)
				sh := cloneShards(full)
				// only the changed old shards are read
				for i := 0; i < k; i++ {
					if newData[i] == nil {
						sh[i] = nil
					}
				}
				if err := c.UpdateParity(sh, newData, p); err != nil {
					t.Fatalf("RS(%d,%d) size %d changed %v: %v", k, m, size, changed, err)
				}
				for j := k; j < k+m; j++ {
					if !bytes.Equal(sh[j], want[j]) {
						t.Fatalf("RS(%d,%d) size %d changed %v: parity %d differs from upstream", k, m, size, changed, j)
					}
				}
				for _, i := range changed { // "the data shards will remain the same"
					if !bytes.Equal(sh[i], full[i]) {
						t.Fatalf("data shard %d was written", i)
					}
				}
				// upstream Update on the same arguments
				up := cloneShards(full)
				if err := cpuUpdateParity(up, newData, k, m); err != nil {
					t.Fatal(err)
				}
				for j := k; j < k+m; j++ {
					if !bytes.Equal(sh[j], up[j]) {
						t.Fatalf("parity %d differs from upstream Update", j)
					}
				}
			}
		}
	}
}

func TestGPUEncodeIdxProgressive(t *testing.T) {
	withGPU(t)
	c := NewCodec()
	p := ErasureProfile{DataShards: 10, ParityShards: 4}
	k, m := p.DataShards, p.ParityShards
	for _, size := range []int{10, 170, 1 << 20, 3<<20 + 17} {
		full, err := c.cpuEncode(randBytes(int64(size), size), p)
		if err != nil {
			t.Fatal(err)
		}
		S := len(full[0])
		parity := make([][]byte, m)
		for j := range parity {
			parity[j] = make([]byte, S)
		}
		for _, i := range []int{7, 0, 9, 3, 1, 8, 2, 6, 4, 5} {
			if err := c.EncodeIdx(full[i], i, parity, p); err != nil {
				t.Fatalf("size %d idx %d: %v", size, i, err)
			}
		}
		for j := range parity {
			if !bytes.Equal(parity[j], full[k+j]) {
				t.Fatalf("size %d: parity %d differs from Encode", size, j)
			}
		}
	}
}

func TestGPUUpdateBatchAndErrors(t *testing.T) {
	withGPU(t)
	c := NewCodec()
	p := ErasureProfile{DataShards: 10, ParityShards: 4}
	k, m := p.DataShards, p.ParityShards
	var shards, news, wants [][][]byte
	for b, size := range []int{10, 1000, 1 << 20, 40000, 3<<20 + 17, 77} {
		full, err := c.cpuEncode(randBytes(int64(size), size), p)
		if err != nil {
			t.Fatal(err)
		}
		nd, want := changedCopy(t, c, full, p, [][]int{{0}, {9}, {3, 7}, {}, {0, 1, 2}, {5}}[b], b)
		shards, news, wants = append(shards, cloneShards(full)), append(news, nd), append(wants, want)
	}
	shards[5][5] = nil // a changed shard without its old bytes
	errs := c.UpdateBatch(shards, news, p)
	for b := range shards {
		if b == 5 {
			if !errors.Is(errs[b], reedsolomon.ErrInvalidInput) {
				t.Fatalf("stripe 5: %v, want ErrInvalidInput", errs[b])
			}
			continue
		}
		if errs[b] != nil {
			t.Fatalf("stripe %d: %v", b, errs[b])
		}
		for j := k; j < k+m; j++ {
			if !bytes.Equal(shards[b][j], wants[b][j]) {
				t.Fatalf("stripe %d: parity %d differs from upstream", b, j)
			}
		}
	}
	full, _ := c.cpuEncode(randBytes(1, 4096), p)
	parity := full[k:]
	if err := c.EncodeIdx(full[0], k, parity, p); !errors.Is(err, reedsolomon.ErrInvalidShardIdx) {
		t.Fatalf("idx k: %v, want ErrInvalidShardIdx", err)
	}
	if err := c.EncodeIdx(full[0], -1, parity, p); !errors.Is(err, reedsolomon.ErrInvalidShardIdx) {
		t.Fatalf("idx -1: %v, want ErrInvalidShardIdx", err)
	}
	nd := make([][]byte, k)
	nd[2] = full[3]
	sh := cloneShards(full)
	sh[2] = nil
	if err := c.UpdateParity(sh, nd, p); !errors.Is(err, reedsolomon.ErrInvalidInput) {
		t.Fatalf("nil old shard: %v, want ErrInvalidInput", err)
	}
	if err := c.UpdateParity(full, nd, ErasureProfile{DataShards: 0, ParityShards: 2}); !errors.Is(err, ErrInvalidProfile) {
		t.Fatalf("k = 0: %v, want ErrInvalidProfile", err)
	}
}

func TestGPUOverwriteMatchesEncode(t *testing.T) {
	withGPU(t)
	c := NewCodec()
	for _, p := range []ErasureProfile{{DataShards: 4, ParityShards: 2}, {DataShards: 10, ParityShards: 4}} {
		k := p.DataShards
		for _, S := range []int{17, 4097, 1<<20 + 1} {
			obj := randBytes(int64(S), k*S)
			for _, r := range [][2]int{{S + 2, 5}, {S - 3, 7}, {S - 1, 2*S + 2}, {0, 1}, {k*S - 1, 1}, {0, k * S}, {2*S - 2, 5}} {
				full, err := c.cpuEncode(obj, p)
				if err != nil {
					t.Fatal(err)
				}
				data := randBytes(int64(r[0]), r[1])
				newObj := append([]byte(nil), obj...)
				copy(newObj[r[0]:], data)
				want, _ := c.cpuEncode(newObj, p)
				sh := cloneShards(full)
				if err := c.Overwrite(sh, p, int64(r[0]), data); err != nil {
					t.Fatalf("RS(%d,%d) S %d range %v: %v", k, p.ParityShards, S, r, err)
				}
				for i := range sh {
					if !bytes.Equal(sh[i], want[i]) {
						t.Fatalf("RS(%d,%d) S %d range %v: shard %d differs from Encode", k, p.ParityShards, S, r, i)
					}
				}
				cpu := cloneShards(full)
				if err := cpuOverwrite(cpu, k, p.ParityShards, int64(r[0]), data); err != nil {
					t.Fatal(err)
				}
				for i := range cpu {
					if !bytes.Equal(cpu[i], want[i]) {
						t.Fatalf("cpuOverwrite: shard %d differs from Encode", i)
					}
				}
			}
			full, _ := c.cpuEncode(obj, p)
			if err := c.Overwrite(full, p, int64(k*S), []byte{1}); err == nil {
				t.Fatal("a range past the object was accepted")
			}
			if err := c.Overwrite(full, p, 0, nil); err == nil {
				t.Fatal("an empty range was accepted")
			}
		}
	}
}
