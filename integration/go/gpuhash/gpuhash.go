// Package gpuhash is the cgo binding a maintainer adds next to the reference's
// src/github.com/cmu440/bitcoin package so the miner's min-hash loop (the TODO at
// src/github.com/cmu440/bitcoin/miner/miner.go:15, spec'd in p1.pdf pp.12-14) runs on
// MI355X GPUs through include/gpuhash.h.  bitcoin.Hash (hash.go:11-15) and the
// Message types (message.go) are untouched.
//
// NOT COMPILED IN THIS REPO: neither the build container nor the GPU box has a Go
// toolchain (DESIGN.md, "Oracle").  Build with:
//
//	CGO_CFLAGS="-I<repo>/include" CGO_LDFLAGS="-L<repo>/bitcoin-miner_amd/lib -lgpuhash" go build
package gpuhash

/*
#cgo LDFLAGS: -lgpuhash
#include <stdlib.h>
#include "gpuhash.h"
*/
import "C"

import (
	"context"
	"unsafe"
)

// Engine owns one gpuhash context (one or more GPUs).
type Engine struct{ ctx *C.gpuhash_ctx }

// Error is a negative gpuhash return code (include/gpuhash.h).
type Error struct {
	Code int
	Msg  string
}

func (e *Error) Error() string { return e.Msg }

// IsArgument reports a deterministic argument error (GPUHASH_EINVAL, GPUHASH_ETOOLONG):
// the same job fails the same way on every miner.  Other codes (ENODEV, EHIP, ENOMEM)
// are device or resource failures.  The miner exits on either kind (miner.go): a server
// pairs each Result with the miner's oldest job, so a skipped job would stay in flight;
// the server's requeue cap then ends a job that fails on every miner.
func (e *Error) IsArgument() bool {
	return e.Code == int(C.GPUHASH_EINVAL) || e.Code == int(C.GPUHASH_ETOOLONG)
}

func rcErr(rc C.int) error {
	if rc == C.GPUHASH_OK {
		return nil
	}
	return &Error{Code: int(rc), Msg: C.GoString(C.gpuhash_strerror(rc))}
}

// Open opens the given HIP device ordinals (none = every visible device).
func Open(devices ...int) (*Engine, error) {
	var ctx *C.gpuhash_ctx
	var rc C.int
	if len(devices) == 0 {
		rc = C.gpuhash_open(nil, 0, &ctx)
	} else {
		ds := make([]C.int, len(devices))
		for i, d := range devices {
			ds[i] = C.int(d)
		}
		rc = C.gpuhash_open(&ds[0], C.int(len(ds)), &ctx)
	}
	if err := rcErr(rc); err != nil {
		return nil, err
	}
	return &Engine{ctx: ctx}, nil
}

// Min returns the least bitcoin.Hash(data, n) over the inclusive [lower, upper] and
// its nonce (lowest nonce on equal hashes) -- exactly what the spec'd loop
//
//	for n := lower; n <= upper; n++ { if h := bitcoin.Hash(data, n); h < best { ... } }
//
// returns.  The cgo call releases the P, so LSP's epoch goroutines keep running.
func (e *Engine) Min(data string, lower, upper uint64) (hash, nonce uint64, err error) {
	var h, n C.uint64_t
	var p *C.uint8_t
	if len(data) > 0 {
		b := []byte(data) // Go-owned, valid for the duration of the call (cgo rules)
		p = (*C.uint8_t)(unsafe.Pointer(&b[0]))
		rc := C.gpuhash_min(e.ctx, p, C.size_t(len(b)), C.uint64_t(lower), C.uint64_t(upper), &h, &n)
		return uint64(h), uint64(n), rcErr(rc)
	}
	rc := C.gpuhash_min(e.ctx, nil, 0, C.uint64_t(lower), C.uint64_t(upper), &h, &n)
	return uint64(h), uint64(n), rcErr(rc)
}

// Cancel stops the search in flight on the engine, from any goroutine, and every search after
// it until Resume: they return an *Error with IsCancelled() true (gpuhash_cancel: a latch, one
// atomic store, no lock).
func (e *Engine) Cancel() error { return rcErr(C.gpuhash_cancel(e.ctx)) }

// Resume clears the latch: searches started after it returns run normally.
func (e *Engine) Resume() error { return rcErr(C.gpuhash_resume(e.ctx)) }

// Progress reports how far the search in flight is: total its nonce count, done an estimate of
// the nonces handed out to the device, which never decreases within a call; (0, 0) when no
// search is in flight.  It does not wait for the search.
func (e *Engine) Progress() (done, total uint64, err error) {
	var d, t C.uint64_t
	rc := C.gpuhash_progress(e.ctx, &d, &t)
	return uint64(d), uint64(t), rcErr(rc)
}

// IsCancelled reports GPUHASH_ECANCELED: the search was stopped by Cancel, nothing failed.
func (e *Error) IsCancelled() bool { return e.Code == int(C.GPUHASH_ECANCELED) }

// MinContext is Min under a context.Context: when ctx is done the search in flight is
// cancelled, within milliseconds, and ctx.Err() is returned.  The latch is cleared before
// MinContext returns, so the engine is usable again.  One MinContext at a time per engine: the
// latch belongs to the engine, not to the call.
func (e *Engine) MinContext(ctx context.Context, data string, lower, upper uint64) (hash, nonce uint64, err error) {
	if err := ctx.Err(); err != nil {
		return 0, 0, err
	}
	finished := make(chan struct{})
	watcher := make(chan struct{})
	go func() {
		defer close(watcher)
		select {
		case <-ctx.Done():
			e.Cancel()
		case <-finished:
		}
	}()
	hash, nonce, err = e.Min(data, lower, upper)
	close(finished)
	<-watcher // no Cancel may follow the Resume
	e.Resume()
	if ge, ok := err.(*Error); ok && ge.IsCancelled() && ctx.Err() != nil {
		return 0, 0, ctx.Err()
	}
	return hash, nonce, err
}

// FirstBelow returns the lowest nonce n of the inclusive [lower, upper] with
// bitcoin.Hash(data, n) <= target, and its hash -- what the ascending loop
//
//	for n := lower; n <= upper; n++ { if h := bitcoin.Hash(data, n); h <= target { return h, n } }
//
// returns; found is false when no nonce of the range qualifies.  The engine stops
// hashing once a hit is known, so an early hit returns early.
func (e *Engine) FirstBelow(data string, lower, upper, target uint64) (hash, nonce uint64, found bool, err error) {
	var h, n C.uint64_t
	var f C.int
	var p *C.uint8_t
	b := []byte(data) // Go-owned, valid for the duration of the call (cgo rules)
	if len(b) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&b[0]))
	}
	rc := C.gpuhash_first_below(e.ctx, p, C.size_t(len(b)), C.uint64_t(lower), C.uint64_t(upper), C.uint64_t(target), &h, &n, &f)
	return uint64(h), uint64(n), f != 0, rcErr(rc)
}

// CollectBelow returns how many nonces n of the inclusive [lower, upper] have
// bitcoin.Hash(data, n) <= target, and the lowest max of them with their hashes, ascending
// by nonce -- what the loop
//
//	for n := lower; n <= upper; n++ { if h := bitcoin.Hash(data, n); h <= target { total++; ... } }
//
// collects.  max is at most GPUHASH_COLLECT_MAX; max == 0 only counts.  Every nonce is
// hashed: the call is built for sparse hits (a pool miner's shares).
func (e *Engine) CollectBelow(data string, lower, upper, target uint64, max int) (total uint64, nonces, hashes []uint64, err error) {
	var t C.uint64_t
	var p *C.uint8_t
	var pn, ph *C.uint64_t
	b := []byte(data) // Go-owned, valid for the duration of the call (cgo rules)
	if len(b) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&b[0]))
	}
	if max < 0 || max > int(C.GPUHASH_COLLECT_MAX) {
		return 0, nil, nil, rcErr(C.GPUHASH_EINVAL)
	}
	if max > 0 {
		nonces = make([]uint64, max)
		hashes = make([]uint64, max)
		pn = (*C.uint64_t)(unsafe.Pointer(&nonces[0]))
		ph = (*C.uint64_t)(unsafe.Pointer(&hashes[0]))
	}
	rc := C.gpuhash_collect_below(e.ctx, p, C.size_t(len(b)), C.uint64_t(lower), C.uint64_t(upper), C.uint64_t(target), pn, ph, C.size_t(max), &t)
	if err = rcErr(rc); err != nil {
		return 0, nil, nil, err
	}
	k := uint64(max)
	if uint64(t) < k {
		k = uint64(t)
	}
	return uint64(t), nonces[:k], hashes[:k], nil
}

// Job is one search of a batch: the inclusive [Lower, Upper] of Data.
type Job struct {
	Data         string
	Lower, Upper uint64
}

// MinBatch answers many independent searches in one call: hashes[k], nonces[k] are exactly
// what Min(jobs[k].Data, jobs[k].Lower, jobs[k].Upper) returns.  For many small jobs (a
// server's chunks, config-1-sized requests): the engine runs one kernel launch per kernel
// variant among all the jobs, where a loop of Min calls pays ~70 us per call.  At most
// GPUHASH_BATCH_MAX_JOBS jobs of at most GPUHASH_BATCH_MAX_SPAN nonces each.
// The ABI takes flat arrays (no Go pointer inside memory passed to C): the messages end to
// end, their offsets, and the bounds.
func (e *Engine) MinBatch(jobs []Job) (hashes, nonces []uint64, err error) {
	n := len(jobs)
	if n == 0 || n > int(C.GPUHASH_BATCH_MAX_JOBS) {
		return nil, nil, rcErr(C.GPUHASH_EINVAL)
	}
	off := make([]C.size_t, n+1)
	lower := make([]C.uint64_t, n)
	upper := make([]C.uint64_t, n)
	msgs := make([]byte, 0, 64*n)
	for k, j := range jobs {
		msgs = append(msgs, j.Data...)
		off[k+1] = C.size_t(len(msgs))
		lower[k] = C.uint64_t(j.Lower)
		upper[k] = C.uint64_t(j.Upper)
	}
	var p *C.uint8_t
	if len(msgs) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&msgs[0]))
	}
	hashes = make([]uint64, n)
	nonces = make([]uint64, n)
	rc := C.gpuhash_min_batch(e.ctx, p, &off[0], C.size_t(n), &lower[0], &upper[0], (*C.uint64_t)(unsafe.Pointer(&hashes[0])), (*C.uint64_t)(unsafe.Pointer(&nonces[0])))
	if err = rcErr(rc); err != nil {
		return nil, nil, err
	}
	return hashes, nonces, nil
}

// FirstBelowBatch answers many independent first-hit searches in one call: found[k], and when
// it is true hashes[k], nonces[k], are exactly what FirstBelow(jobs[k].Data, jobs[k].Lower,
// jobs[k].Upper, targets[k]) returns -- the lowest nonce whose hash is at or below the target.
// For a service that mints one proof-of-work stamp per request: the engine runs one kernel
// launch per digit count and kernel variant among all the jobs, in ascending digit order, so
// a job with an early hit costs next to nothing, where a loop of FirstBelow calls pays
// ~0.4 ms per call.  len(targets) must equal len(jobs); the limits are MinBatch's.
func (e *Engine) FirstBelowBatch(jobs []Job, targets []uint64) (hashes, nonces []uint64, found []bool, err error) {
	n := len(jobs)
	if n == 0 || n > int(C.GPUHASH_BATCH_MAX_JOBS) || len(targets) != n {
		return nil, nil, nil, rcErr(C.GPUHASH_EINVAL)
	}
	off := make([]C.size_t, n+1)
	lower := make([]C.uint64_t, n)
	upper := make([]C.uint64_t, n)
	target := make([]C.uint64_t, n)
	msgs := make([]byte, 0, 64*n)
	for k, j := range jobs {
		msgs = append(msgs, j.Data...)
		off[k+1] = C.size_t(len(msgs))
		lower[k] = C.uint64_t(j.Lower)
		upper[k] = C.uint64_t(j.Upper)
		target[k] = C.uint64_t(targets[k])
	}
	var p *C.uint8_t
	if len(msgs) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&msgs[0]))
	}
	hashes = make([]uint64, n)
	nonces = make([]uint64, n)
	f := make([]C.int, n)
	rc := C.gpuhash_first_below_batch(e.ctx, p, &off[0], C.size_t(n), &lower[0], &upper[0], &target[0], (*C.uint64_t)(unsafe.Pointer(&hashes[0])), (*C.uint64_t)(unsafe.Pointer(&nonces[0])), &f[0])
	if err = rcErr(rc); err != nil {
		return nil, nil, nil, err
	}
	found = make([]bool, n)
	for k := range f {
		found[k] = f[k] != 0
	}
	return hashes, nonces, found, nil
}

// JobHits is one job's answer of CollectBelowBatch: the exact number of qualifying nonces, and the
// lowest min(cap, Total) of them, ascending, with their hashes.
type JobHits struct {
	Total  uint64
	Nonces []uint64
	Hashes []uint64
}

// CollectBelowBatch answers many independent collections in one call: out[k] is exactly what
// CollectBelow(jobs[k].Data, jobs[k].Lower, jobs[k].Upper, targets[k], caps[k]) returns -- the
// exact hit count and the lowest caps[k] hits.  For a miner that holds many short work units,
// each with its own share target: the engine runs one kernel launch per kernel variant among
// all the jobs, where a loop of CollectBelow calls pays ~0.1 ms per call.  Built for sparse
// hits.  caps == nil only counts; else len(caps) and len(targets) must equal len(jobs) and
// every cap be at most GPUHASH_COLLECT_MAX; the other limits are MinBatch's.
func (e *Engine) CollectBelowBatch(jobs []Job, targets []uint64, caps []int) (out []JobHits, err error) {
	n := len(jobs)
	if n == 0 || n > int(C.GPUHASH_BATCH_MAX_JOBS) || len(targets) != n || (caps != nil && len(caps) != n) {
		return nil, rcErr(C.GPUHASH_EINVAL)
	}
	off := make([]C.size_t, n+1)
	lower := make([]C.uint64_t, n)
	upper := make([]C.uint64_t, n)
	target := make([]C.uint64_t, n)
	totals := make([]uint64, n)
	msgs := make([]byte, 0, 64*n)
	for k, j := range jobs {
		msgs = append(msgs, j.Data...)
		off[k+1] = C.size_t(len(msgs))
		lower[k] = C.uint64_t(j.Lower)
		upper[k] = C.uint64_t(j.Upper)
		target[k] = C.uint64_t(targets[k])
	}
	var p *C.uint8_t
	if len(msgs) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&msgs[0]))
	}
	var outOff []C.size_t
	var po *C.size_t
	var pn, ph *C.uint64_t
	var nonces, hashes []uint64
	if caps != nil {
		outOff = make([]C.size_t, n+1)
		for k, c := range caps {
			if c < 0 || c > int(C.GPUHASH_COLLECT_MAX) {
				return nil, rcErr(C.GPUHASH_EINVAL)
			}
			outOff[k+1] = outOff[k] + C.size_t(c)
		}
		po = &outOff[0]
		if room := int(outOff[n]); room > 0 {
			nonces = make([]uint64, room)
			hashes = make([]uint64, room)
			pn = (*C.uint64_t)(unsafe.Pointer(&nonces[0]))
			ph = (*C.uint64_t)(unsafe.Pointer(&hashes[0]))
		}
	}
	rc := C.gpuhash_collect_below_batch(e.ctx, p, &off[0], C.size_t(n), &lower[0], &upper[0], &target[0], po, pn, ph, (*C.uint64_t)(unsafe.Pointer(&totals[0])))
	if err = rcErr(rc); err != nil {
		return nil, err
	}
	out = make([]JobHits, n)
	for k := range out {
		out[k].Total = totals[k]
		if caps == nil {
			continue
		}
		at, held := int(outOff[k]), caps[k]
		if totals[k] < uint64(held) {
			held = int(totals[k])
		}
		out[k].Nonces = nonces[at : at+held]
		out[k].Hashes = hashes[at : at+held]
	}
	return out, nil
}

// Close releases the devices.
func (e *Engine) Close() { C.gpuhash_close(e.ctx) }
