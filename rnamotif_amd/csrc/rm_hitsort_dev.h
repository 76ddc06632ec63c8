// rm_hitsort_dev.h -- the hit records into the reference's output order on the device.
//
// Same result as rma::sort_hits() (rm_hitsort.h, which says what the order is and why): the five
// header words packed into one 64-bit key of the widths this database and descriptor need, a
// stable radix sort of (key, slot in the hit buffer) pairs -- rocPRIM's, a plain library sort --
// then one kernel that moves the records and renumbers the order word.  The copy back is then
// the final, ordered stream and the host does not touch the records at all (its sort + gather took
// 0.3 ms of a 4.4 ms step at 100 Mbase, 1.9 of 38 ms at 1 Gbase).  A record whose header does not
// fit the key is flagged and the caller falls back to the host sort.
#pragma once
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdint>
#include "rm_hip_own.h"

namespace rma {

#define RANK_SORT_MAX	8192	// pairs up to which the ordering sorts by its own counting kernel, beyond it by rocPRIM (rm_hitsort_dev.hip)

struct DevHitSort {
	DevMem	keys[ 2 ], vals[ 2 ];	// 64-bit keys and 32-bit slots, before and after the sort
	DevMem	tmp;			// the library's work area
	DevMem	out, flag;		// the ordered records, one 64-bit word
	int64_t	cap = 0;		// records there is room for: all six buffers or none (0)
	int	stride = 0;
	int	w_ord = 20;	// bits for the order word (pieces of items count in their own ranges, rm_scan_kernel.h PIECE_ORDER_BITS); widened after a scan whose order words did not fit
	// The flag is raised by a run storing its own number there, and runs are numbered from 1: the word is cleared once, when
	// it is made, and no run has to clear it (a memset on the stream in front of every ordering, before).
	unsigned long long	epoch = 0;	// the number of the last run: the flag word holds it if that run raised the flag

	int32_t	*d_out() const { return out.as<int32_t>(); }
	unsigned long long	*d_flag() const { return flag.as<unsigned long long>(); }
	// room for cap records of stride words; on failure the object is as release() leaves it: cap 0, no buffer
	hipError_t	reserve( int64_t cap, int stride );
	// Enqueue on s: d_out[ n ][ stride ] = d_hits[ n ][ stride ] in order, order word renumbered;
	// *d_flag == epoch afterwards if some header word did not fit (then d_out is not to be used).
	// Returns hipErrorInvalidValue without enqueuing anything when the widths leave no room for
	// the order word.
	hipError_t	run( const int32_t *d_hits, int64_t n, int w_seq, int w_pos, int w_rank, hipStream_t s );
	// The same enqueued before the host knows the count (rm_tail_plan.h): sized for n records, of which min( *d_count, n ) are
	// there when it runs (d_count null: n).  The flag goes to d_flag_word, a word the caller has cleared or that holds an
	// earlier run's number; with h_out, page-locked memory, the ordered records are stored there too.  plan( n ) comes first,
	// while nothing that the sort's work area serves is enqueued: run() of this form neither waits nor allocates.
	hipError_t	plan( int64_t n, hipStream_t s );
	// the key has room for these fields and four bits of the order word at least: run() does not refuse them
	bool	widths_ok( int w_seq, int w_pos, int w_rank ) const
	{
		return w_seq <= 31 && w_pos <= 31 && w_rank <= 31 && std::min( { w_ord, 31, 64 - ( w_seq + 1 + w_pos + w_rank ) } ) >= 4;
	}
	hipError_t	run( const int32_t *d_hits, int64_t n, const unsigned long long *d_count, unsigned long long *d_flag_word, int32_t *h_out,
		int w_seq, int w_pos, int w_rank, hipStream_t s );
	void	release();
};

// word 0 of every record (the entry's number within one scan's database) becomes index[ word 0 ], the
// entry's number in the whole database: what a rank of a multi-GPU search does before its records
// travel (rm_gather.cpp).  Records whose word 0 is outside 0 .. n_index-1 are left as they are.
hipError_t	relabel_entries( int32_t *d_hits, int64_t n, int stride, const int32_t *d_index, int32_t n_index, hipStream_t s );

}	// namespace rma
