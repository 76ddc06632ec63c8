// rm_hitprint_dev.h -- hit records as rnamotif prints them, on the device (rma_hit_print, rm_hitpost.cpp).  The rule
// is rm_hitprint.h's, shared with the host.
//
//   rma_hit_print_size_kernel  one lane per record: checks it (hitwin_span's checks, then its text_len), the bytes of
//                              its two lines, 0 where accept[ h ] is false or the record is bad; the index of a bad
//                              record and of a bad text_len go into two words by an atomic minimum
//   exclusive scan             of the sizes into 64-bit offsets (rocPRIM, hit_offsets of rm_hitwin_dev.h)
//   rma_hit_print_kernel       one wave per record: lane k computes segment k and 64 + k of the lines, a wave-wide
//                              prefix over their lengths puts the segments' first bytes into LDS; the digits of comp,
//                              offset and len are made once, by one lane, into LDS; then the lanes take consecutive
//                              bytes of the lines, find each one's segment by bisection and store it: the stores of a
//                              wave are one run of the output, the text reads of a field one run of the entry,
//                              descending on strand 1
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "rm_hitprint.h"

namespace rma {

// the names of a database's entries in device memory: the sid of entry e is bytes [ off[ 2e ], off[ 2e + 1 ] ), its
// sdef bytes [ off[ 2e + 1 ], off[ 2e + 2 ] )
struct HitPrintNames {
	const uint8_t	*bytes;
	const int64_t	*off;
};

// records [0, n) of a call, the call's record `first` the first of them; accept may be null (all)
struct HitPrintBatch {
	const int32_t	*hits;
	long long	n, first;
	int	stride;
	HitWinShape	shape;
	const int32_t	*slen;
	const int64_t	*start;
	int32_t	n_seq;
	const uint8_t	*accept;
	const int32_t	*text_len;
	int32_t	text_width;
	HitPrintNames	names;
};

// Enqueue on s: d_len[ h ] = the bytes of record h's lines (0: not accepted, or bad), d_len[ n ] = 0;
// *d_bad = min( *d_bad, first + h ) for a record that fails hitwin_span's checks, *d_bad_text likewise for one whose
// text_len lies outside [0, text_width].
hipError_t	hit_print_sizes( const HitPrintBatch &b, int64_t *d_len, unsigned long long *d_bad, unsigned long long *d_bad_text, hipStream_t s );

// Enqueue on s: the lines of records [0, n), record h's d_offc[ h + 1 ] - d_offc[ h ] bytes at d_out + *d_carry +
// d_offc[ h ], and d_off[ h ] = *d_carry + d_offc[ h ] (last: d_off[ n ] too); the caller has seen both bad words
// untouched.  text, table and codes as hit_gather takes them; text_bytes: the score columns of the whole call, rows of
// text_width bytes -- record h of the batch reads row b.first + h.
hipError_t	hit_print_fill( const HitPrintBatch &b, const uint8_t *text, const uint8_t *table, int codes, const uint8_t *text_bytes,
	const int64_t *d_offc, const int64_t *d_carry, uint8_t *d_out, int64_t *d_off, bool last, hipStream_t s );

}	// namespace rma
