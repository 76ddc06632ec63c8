// rm_hitlist_dev.h -- hit records as rmfmt lists them, on the device (rma_hit_list, rm_hitpost.cpp).  The rule is
// rm_hitlist.h's, shared with the host.
//
//   rma_hit_list_measure_kernel  one lane per record: checks it (hitprint_check, then the rule's own refusals),
//                                tokenises its score column, trims its entry's name, keeps a HitListRec of it and a
//                                flag for the compaction; the column maxima, the 64-bit sum of the temp lines, the
//                                least and greatest number of score fields, whether some token is no number and the
//                                least refused record with its code are reduced within the wave and leave it as one
//                                atomic per wave and word
//   exclusive scan, compact      the flags into offsets (rocPRIM, hit_offsets of rm_hitwin_dev.h); the printed
//                                records' indices in input order
//   sort                         rocprim::merge_sort of the indices under rmlist_less (modes 1 and 2)
//   rma_hit_list_fill_kernel     one wave per line: the layout's offsets lie in LDS once per workgroup -- they are
//                                the same for every line --, the lengths of the line's own segments once per line;
//                                lanes take consecutive bytes of the line, find each one's segment by bisection and
//                                store it: the stores of a wave are one run of the row
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "rm_hitlist.h"
#include "rm_hitprint_dev.h"

namespace rma {

// what the measure pass reduces over a call; `init` is what it starts from
struct HitListSums {
	unsigned long long	bad;		// min( record * 16 + code ) over the refused records
	unsigned long long	first;		// the least printed record
	unsigned long long	temp_bytes, n_lines;
	uint32_t	k_min, k_max, not_number, pad_;
	uint32_t	width[ HL_MAX_SEGS ];
	static HitListSums	init()
	{
		HitListSums	s;
		for( size_t i = 0; i < sizeof( s ); i++ )
			reinterpret_cast<unsigned char *>( &s )[ i ] = 0;
		s.bad = s.first = ~0ull;
		s.k_min = ~0u;
		return s;
	}
};

// the records of a call and what is read with them; accept may be null (all)
struct HitListCall {
	const int32_t	*hits;
	long long	n;
	int	stride;
	HitWinShape	shape;
	const int32_t	*slen;
	const int64_t	*start;
	int32_t	n_seq;
	const uint8_t	*accept;
	const int32_t	*text_len;
	const uint8_t	*text_bytes;
	int32_t	text_width;
	HitPrintNames	names;
	int	name_mode;
	HitListRec	*recs;		// n of them: written by the measure pass, read by the sort and the fill
};

// Enqueue on s, for records [c0, c0 + cn) of the call: their HitListRec, d_flag[ i ] = 1 for record c0 + i when it is
// printed, else 0, d_flag[ cn ] = 0, and the reductions into *d_sums.
hipError_t	hit_list_measure( const HitListCall &c, long long c0, long long cn, int64_t *d_flag, HitListSums *d_sums, hipStream_t s );

// Enqueue on s: d_idx[ *d_carry + d_off[ i ] ] = c0 + i for every i < cn with d_flag[ i ] != 0
hipError_t	hit_list_compact( const int64_t *d_flag, const int64_t *d_off, const int64_t *d_carry, long long c0, long long cn, int64_t *d_idx, hipStream_t s );

// Enqueue on s: d_letcmp[ b ] = the letter of text byte b, d_letcmp[ 256 + b ] its complement (table, codes: as
// hit_gather takes them)
hipError_t	hit_list_letters( const uint8_t *table, int codes, uint8_t *d_letcmp, hipStream_t s );

// d_perm[ n_lines ] = d_idx[ n_lines ] in the order of rmlist_less under mode (1 or 2).  tmp null: *tmp_bytes = the
// work area this sort needs, nothing enqueued.
hipError_t	hit_list_sort( const HitListCall &c, const uint8_t *text, const uint8_t *d_letcmp, int mode, const int64_t *d_idx, int64_t *d_perm,
	long long n_lines, void *tmp, size_t *tmp_bytes, hipStream_t s );

// Enqueue on s: line r of the listing, the l.line_len bytes of record d_perm[ r ], at d_out + r * line_len
hipError_t	hit_list_fill( const HitListCall &c, const uint8_t *text, const uint8_t *d_letcmp, const HitListLayout *d_layout, int32_t line_len,
	const int64_t *d_perm, long long n_lines, uint8_t *d_out, hipStream_t s );

}	// namespace rma
