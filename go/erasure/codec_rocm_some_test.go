//go:build rocm && cgo

package erasure

// DecodeData, DecodeDataBatch and RepairSome against the reference CPU codec and upstream
// ReconstructData / ReconstructSome: objects, errors, and which nil entries are filled.
// Needs a HIP device: `go test -tags rocm ./erasure/` on a GPU box.

import (
	"bytes"
	"errors"
	"testing"
)

func loseShards(full [][]byte, lost ...int) [][]byte {
	s := cloneShards(full)
	for _, i := range lost {
		s[i] = nil
	}
	return s
}

func TestGPUDecodeDataLeavesParityNil(t *testing.T) {
	withGPU(t)
	c := NewCodec()
	p := ErasureProfile{DataShards: 10, ParityShards: 4}
	for _, size := range []int{1, 1000, 1 << 20, 3<<20 + 17} {
		data := randBytes(int64(size), size)
		full, err := c.cpuEncode(data, p)
		if err != nil {
			t.Fatal(err)
		}
		for _, lost := range [][]int{{3}, {0, 12}, {10, 11, 12, 13}, {1, 2, 11, 13}, {}} {
			sh := loseShards(full, lost...)
			got, err := c.DecodeData(sh, p, int64(size))
			if err != nil || !bytes.Equal(got, data) {
				t.Fatalf("size %d lost %v: err %v", size, lost, err)
			}
			ref, rerr := c.Decode(loseShards(full, lost...), p, int64(size))
			if rerr != nil || !bytes.Equal(ref, got) {
				t.Fatalf("size %d lost %v: DecodeData differs from Decode", size, lost)
			}
			for _, i := range lost {
				if i < p.DataShards && !bytes.Equal(sh[i], full[i]) {
					t.Fatalf("size %d lost %v: data shard %d not rebuilt", size, lost, i)
				}
				if i >= p.DataShards && sh[i] != nil {
					t.Fatalf("size %d lost %v: parity shard %d was filled", size, lost, i)
				}
			}
		}
	}
}

func TestGPUDecodeDataErrors(t *testing.T) {
	withGPU(t)
	c := NewCodec()
	p := ErasureProfile{DataShards: 4, ParityShards: 2}
	data := randBytes(7, 1<<20)
	full, _ := c.cpuEncode(data, p)
	for name, sh := range map[string][][]byte{
		"too few":   loseShards(full, 0, 1, 5),
		"no data":   make([][]byte, 6),
		"too short": full[:5],
	} {
		_, got := c.DecodeData(cloneShards(sh), p, int64(len(data)))
		_, want := c.cpuDecode(cloneShards(sh), p, int64(len(data)))
		sameErr(t, name, got, want)
	}
	bad := loseShards(full, 0)
	bad[5] = append([]byte(nil), bad[5]...)
	bad[5][9] ^= 1
	if _, err := c.DecodeData(bad, p, int64(len(data))); !errors.Is(err, ErrShardCorrupted) {
		t.Fatalf("flipped compared shard: %v", err)
	}
	if _, err := c.DecodeData(loseShards(full, 1, 4), p, int64(len(data))+8); !errors.Is(err, ErrInsufficientShards) {
		t.Fatalf("oversized original: %v", err)
	}
}

func TestGPUDecodeDataBatchAndRepairSome(t *testing.T) {
	withGPU(t)
	c := NewCodec()
	p := ErasureProfile{DataShards: 10, ParityShards: 4}
	sizes := []int{100, 70000, 1 << 20, 5, 333333, 2 << 20}
	lost := [][]int{{3}, {10, 11, 12, 13}, {0, 13}, {}, {2, 5, 11}, {0, 1, 2, 3, 4}}
	var fulls [][][]byte
	var datas [][]byte
	batch := make([][][]byte, len(sizes))
	osz := make([]int64, len(sizes))
	for b, size := range sizes {
		data := randBytes(int64(100+b), size)
		full, err := c.cpuEncode(data, p)
		if err != nil {
			t.Fatal(err)
		}
		fulls, datas = append(fulls, full), append(datas, data)
		batch[b] = loseShards(full, lost[b]...)
		osz[b] = int64(size)
	}
	out, errs := c.DecodeDataBatch(batch, p, osz)
	for b := range sizes {
		_, want := c.cpuDecode(loseShards(fulls[b], lost[b]...), p, osz[b])
		sameErr(t, "object", errs[b], want)
		if want != nil {
			continue
		}
		if !bytes.Equal(out[b], datas[b]) {
			t.Fatalf("object %d differs", b)
		}
		for _, i := range lost[b] {
			if i >= p.DataShards && batch[b][i] != nil {
				t.Fatalf("object %d: parity shard %d was filled", b, i)
			}
			if i < p.DataShards && !bytes.Equal(batch[b][i], fulls[b][i]) {
				t.Fatalf("object %d: data shard %d not rebuilt", b, i)
			}
		}
	}
	// a repair that wants one shard index back per object
	objs := make([][][]byte, len(sizes))
	want := make([][]bool, len(sizes))
	for b := range sizes {
		objs[b] = loseShards(fulls[b], lost[b]...)
		want[b] = make([]bool, 14)
		if len(lost[b]) > 0 {
			want[b][lost[b][0]] = true
		}
	}
	rerrs := c.RepairSome(objs, want, p)
	for b := range sizes {
		if len(lost[b]) > p.ParityShards {
			if rerrs[b] == nil {
				t.Fatalf("object %d: too few shards went unreported", b)
			}
			continue
		}
		if rerrs[b] != nil {
			t.Fatalf("object %d: %v", b, rerrs[b])
		}
		for n, i := range lost[b] {
			if n == 0 && !bytes.Equal(objs[b][i], fulls[b][i]) {
				t.Fatalf("object %d: wanted shard %d not rebuilt", b, i)
			}
			if n > 0 && objs[b][i] != nil {
				t.Fatalf("object %d: unwanted shard %d was filled", b, i)
			}
		}
	}
	// want == nil is RepairBatch
	objs[0] = loseShards(fulls[0], 3, 12)
	if errs := c.RepairSome(objs[:1], nil, p); errs[0] != nil || !bytes.Equal(objs[0][12], fulls[0][12]) {
		t.Fatalf("RepairSome(nil): %v", errs[0])
	}
}
