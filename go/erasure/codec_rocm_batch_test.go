//go:build rocm && cgo

package erasure

// EncodeBatch / DecodeBatch against the reference CPU codec (cpuEncode / cpuDecode, i.e.
// klauspost/reedsolomon itself) object by object: the same shards, the same objects, the
// same errors by errors.Is and by text, the same filling of nil entries. Runs where Go, the
// module cache and a HIP device are present (`go test -tags rocm ./erasure/`); where there
// is no Go toolchain, tests/native/codec_batch_drive.c drives the same two C calls.

import (
	"bytes"
	"errors"
	"testing"

	"github.com/klauspost/reedsolomon"
)

func cloneShards(s [][]byte) [][]byte {
	out := make([][]byte, len(s))
	for i := range s {
		if s[i] != nil {
			out[i] = append([]byte(nil), s[i]...)
		}
	}
	return out
}

func sameErr(t *testing.T, what string, got, want error) {
	t.Helper()
	if (got == nil) != (want == nil) {
		t.Fatalf("%s: got %v, reference %v", what, got, want)
	}
	if got == nil {
		return
	}
	if got.Error() != want.Error() {
		t.Fatalf("%s: got %q, reference %q", what, got, want)
	}
	for _, target := range []error{ErrShardCorrupted, ErrInsufficientShards, ErrInvalidProfile,
		reedsolomon.ErrShortData, reedsolomon.ErrTooFewShards, reedsolomon.ErrShardSize,
		reedsolomon.ErrShardNoData} {
		if errors.Is(got, target) != errors.Is(want, target) {
			t.Fatalf("%s: errors.Is(%v) differs: got %v, reference %v", what, target, got, want)
		}
	}
}

func TestGPUEncodeBatchMatchesReference(t *testing.T) {
	withGPU(t)
	c := NewCodec()
	for _, p := range []ErasureProfile{{DataShards: 4, ParityShards: 2}, {DataShards: 10, ParityShards: 4},
		{DataShards: 20, ParityShards: 16}, {DataShards: 1, ParityShards: 3}} {
		k := p.DataShards
		sizes := []int{1, 2, 0, k - 1, k, k + 1, 16*k - 1, 16*k + 1, 8192*k - 1, 8192*k + 1, 1<<20 + 7, 0}
		objs := make([][]byte, len(sizes))
		for b, n := range sizes {
			if n > 0 {
				objs[b] = randBytes(int64(n+k+b), n)
			}
		}
		// one object in a body with room for all its shards: split in place
		if body := BodyBuffer(sizes[10], p); body != nil {
			copy(body, objs[10])
			objs[10] = body
			defer FreeHostBuffer(body)
		}
		want := make([][]byte, len(objs))
		for b := range objs {
			want[b] = append([]byte(nil), objs[b]...)
		}
		got, errs := c.EncodeBatch(objs, p)
		for b := range objs {
			ref, rerr := c.cpuEncode(append([]byte(nil), want[b]...), p)
			sameErr(t, "encode", errs[b], rerr)
			if rerr != nil {
				if got[b] != nil {
					t.Fatalf("object %d: shards beside an error", b)
				}
				continue
			}
			if len(got[b]) != len(ref) {
				t.Fatalf("object %d: %d shards, reference %d", b, len(got[b]), len(ref))
			}
			for i := range ref {
				if !bytes.Equal(got[b][i], ref[i]) {
					t.Fatalf("%+v object %d (%d bytes): shard %d differs from reedsolomon", p, b, sizes[b], i)
				}
			}
			if !bytes.Equal(objs[b][:len(want[b])], want[b]) {
				t.Fatalf("object %d: the input changed", b)
			}
		}
	}
}

func TestGPUDecodeBatchMatchesReference(t *testing.T) {
	withGPU(t)
	c := NewCodec()
	p := ErasureProfile{DataShards: 10, ParityShards: 4}
	k, n := 10, 14
	sizes := []int{1, 17, 4096, 99_991, 1<<20 + 3, 160, 161, 5000, 5001, 77, 78, 3000}
	objs := make([][]byte, len(sizes))
	for b, sz := range sizes {
		objs[b] = randBytes(int64(sz+b), sz)
	}
	enc, errs := c.EncodeBatch(objs, p)
	for b := range errs {
		if errs[b] != nil {
			t.Fatal(errs[b])
		}
	}
	batch := make([][][]byte, len(sizes))
	orig := make([]int64, len(sizes))
	for b := range enc {
		batch[b] = cloneShards(enc[b])
		orig[b] = int64(sizes[b])
		S := len(enc[b][0])
		switch b {
		case 0: // nothing missing
		case 1:
			batch[b][0] = nil
		case 2:
			batch[b][k] = nil
		case 3:
			batch[b][0], batch[b][3], batch[b][7], batch[b][12] = nil, nil, nil, nil
		case 4:
			batch[b][0], batch[b][1], batch[b][2], batch[b][3] = nil, nil, nil, nil
		case 5: // k-1 present
			for i := 0; i < 5; i++ {
				batch[b][i] = nil
			}
		case 6: // a shard of another length
			batch[b][2] = batch[b][2][:S-1]
		case 7: // every entry nil
			batch[b] = make([][]byte, n)
		case 8: // a flipped byte in a compared parity shard
			batch[b][1] = nil
			batch[b][n-1][S/2] ^= 0x40
		case 9: // originalSize beyond k*S
			orig[b] = int64(k*S + 1)
		case 10: // the same with the flipped byte: corruption is reported first
			orig[b] = int64(k*S + 1)
			batch[b][n-1][0] ^= 1
		case 11: // a wrong shard count
			batch[b] = batch[b][:n-1]
		}
	}
	alone := make([][][]byte, len(batch))
	for b := range batch {
		alone[b] = cloneShards(batch[b])
	}
	got, derrs := c.DecodeBatch(batch, p, orig)
	for b := range batch {
		ref, rerr := c.cpuDecode(alone[b], p, orig[b])
		sameErr(t, "decode", derrs[b], rerr)
		if rerr == nil && !bytes.Equal(got[b], ref) {
			t.Fatalf("object %d: joined bytes differ from the reference", b)
		}
		if rerr != nil && got[b] != nil {
			t.Fatalf("object %d: an object beside an error", b)
		}
		for i := range alone[b] {
			if !bytes.Equal(batch[b][i], alone[b][i]) || (batch[b][i] == nil) != (alone[b][i] == nil) {
				t.Fatalf("object %d: entry %d filled differently from upstream Reconstruct", b, i)
			}
		}
	}
	// an empty object and an empty batch
	out, e2 := c.DecodeBatch([][][]byte{cloneShards(enc[3])}, p, []int64{0})
	if e2[0] != nil || len(out[0]) != 0 {
		t.Fatalf("original size 0: %v, %d bytes", e2[0], len(out[0]))
	}
	if o, e := c.DecodeBatch(nil, p, nil); len(o) != 0 || len(e) != 0 {
		t.Fatal("an empty batch returns empty results")
	}
}
