// rm_hitct_dev.h -- hit records as rm2ct writes them, on the device (rma_hit_ct, rm_hitpost.cpp).  The rule is
// rm_hitct.h's, shared with the host.  Both kernels give a record to a wave and begin alike: the record checked
// (hitprint_check); where it is accepted its score column searched for a newline, its hit line measured and, for rnaviz,
// its energy read, by one lane (hitct_measure); the prefix of its field lengths laid into LDS by a wave-wide prefix sum.
//
//   rma_hit_ct_size_kernel  lane l adds up the record's lines l, l + 64, ... (hitct_size_part), the wave reduces them:
//                           the record's bytes, 0 where accept[ h ] is false or the record is refused; the least
//                           refused record goes into a word with its reason, ( index << 4 ) | code, by an atomic minimum
//   exclusive scan          of the sizes into 64-bit offsets (rocPRIM, hit_offsets of rm_hitwin_dev.h)
//   rma_hit_ct_kernel       the header line's two halves are formatted once, by one lane, into LDS and copied out around
//                           the name by all; then the lanes take the bases' lines in passes of 64: each lane finds its
//                           base's field by bisection in the prefix, formats its line once into its slot in LDS, a
//                           wave-wide prefix sum of the lengths, carried from pass to pass, places the lines, and the
//                           wave writes the pass out as one run of bytes, each lane finding its byte's line by bisection
//                           in the pass's offsets.  No workgroup barrier stands in the loop over records: what one
//                           wave's lanes hand each other through LDS is ordered by wave barriers.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "rm_hitct.h"
#include "rm_hitprint_dev.h"

namespace rma {

// records [0, b.n) of a call as rma_hit_print takes them, with their score columns (the call's rows: record h of the
// batch reads row b.first + h), the output's type and the descriptor's table
struct HitCtBatch {
	HitPrintBatch	b;
	const uint8_t	*text_bytes;
	int32_t	type;
	HitCtTable	table;
};

// Enqueue on s: d_len[ h ] = the bytes of record h's .ct record (0: not accepted, or refused), d_len[ n ] = 0;
// *d_bad = min( *d_bad, ( first + h ) << 4 | code ) for a record hitprint_check or hitct_measure refuses.
hipError_t	hit_ct_sizes( const HitCtBatch &c, int64_t *d_len, unsigned long long *d_bad, hipStream_t s );

// Enqueue on s: the .ct records of records [0, n), record h's d_offc[ h + 1 ] - d_offc[ h ] bytes at d_out + *d_carry +
// d_offc[ h ], and d_off[ h ] = *d_carry + d_offc[ h ] (last: d_off[ n ] too); the caller has seen *d_bad untouched.
// text, table and codes as hit_gather takes them.
hipError_t	hit_ct_fill( const HitCtBatch &c, const uint8_t *text, const uint8_t *table, int codes, const int64_t *d_offc, const int64_t *d_carry,
	uint8_t *d_out, int64_t *d_off, bool last, hipStream_t s );

}	// namespace rma
