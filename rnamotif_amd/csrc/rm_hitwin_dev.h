// rm_hitwin_dev.h -- the windows of hit records cut out of a device database's text on the device
// (rma_replay_device, rm_hitpost.cpp).  The rule is rm_hitwin.h's, shared with the host.
//
//   rma_hit_span_kernel    one lane per record: checks it, its window's length (0 for a bad record, whose index
//                          goes into *bad by an atomic minimum), the span's first position
//   exclusive scan         of the lengths into 64-bit offsets (rocPRIM)
//   rma_hit_gather_kernel  one wave per record: the letters of its window through a table in LDS, lanes over
//                          consecutive bytes, on strand 1 read from the 3' end and complemented
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "rm_hitwin.h"

namespace rma {

// Enqueue on s: for records [0, n) at d_hits (stride words each), d_len[ h ] = the window's length, d_lo[ h ] its
// first position in the strand and d_src[ h ] its first byte in the text (strand 1: -1 - that byte, the window read
// downwards from it), d_len[ n ] = 0 (the three may be null: the checks alone); *d_bad = min( *d_bad, h ) for every
// record h that fails a check (its length 0).  d_slen, d_start: the database's n_seq entry lengths and starts.
hipError_t	hit_spans( const int32_t *d_hits, int64_t n, int stride, const HitWinShape &shape, const int32_t *d_slen,
	const int64_t *d_start, int32_t n_seq, int32_t *d_lo, int64_t *d_len, int64_t *d_src, unsigned long long *d_bad, hipStream_t s );

// d_off[ 0 .. n ] = the exclusive sum of d_len[ 0 .. n ]; tmp == null: *tmp_bytes receives the room it needs
hipError_t	hit_offsets( const int64_t *d_len, int64_t *d_off, int64_t n_plus_1, void *tmp, size_t *tmp_bytes, hipStream_t s );

// Enqueue on s: the windows of records [0, n) into d_out, record h's d_off[ h + 1 ] - d_off[ h ] bytes from d_src[ h ]
// (hit_spans) at d_out + d_off[ h ] - d_off[ 0 ]; the caller has seen *d_bad untouched.  table: 256 bytes in device
// memory, the letter of each byte (codes = 0) or the code of each byte, 0-3 for acgt (codes = 1).
hipError_t	hit_gather( const uint8_t *text, int64_t n, const int64_t *d_src, const int64_t *d_off, const uint8_t *table, int codes,
	uint8_t *d_out, hipStream_t s );

}	// namespace rma
