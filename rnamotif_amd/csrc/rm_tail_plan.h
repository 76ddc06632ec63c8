// rm_tail_plan.h -- the rule by which a scan's tail (energies, ordering, copy back) is enqueued behind its search and
// drain kernels before the host knows how many records there are, and the rule by which rma_scan_end() then takes what
// the tail left or does the tail again as it always did.  Plain C++, no HIP call: rm_scanner.cpp owns the resources and
// calls these; tests/hostsim/tail_plan_check.cpp holds them on the CPU.
//
// The tail is sized on the host by a planned count, n_sort, and on the device by the count the kernels in front of it
// left in HBM: the energy and gather kernels stop at the count, the keys beyond it are padding that sorts last.  A scan
// with more records than planned, or one that search_finish() would repeat, is not harmed by the tail that ran: the
// energy words are written from a record's other words only, and the ordering writes buffers of its own.
#pragma once
#include <algorithm>
#include <cstdint>

namespace rma {

struct TailOpts {
	int	spec_tail = -1;		// option spec_tail: -1 by the rule, 0 never
	int	dbg = 0, timing = 0, host_sort = 0;	// each of them wants the tail in its steps, as it was
	bool	timed_apart = false;	// rma_scan_device(): the kernels timed apart, one energy launch behind a wait
};

struct TailPlan {
	bool	speculate = false;
	int64_t	n_sort = 0;		// records the ordering and the copy back are sized for
};

#define RMA_TAIL_MIN	1024		// records planned for at least: a kernel of the ordering does not get cheaper below it

// What a scanner remembers of the counts of the scans it has ended, for plan_tail(): the last scan's count, or half of what it
// remembered where that is more -- one scan with many records does not size the tails of all the scans after it (the ordering
// and the energy grid are paid for the planned size, whatever is found): the plan halves from scan to scan until it meets
// the counts again.  A steady sequence of scans keeps its plan; one that falls by more than half a scan keeps being taken.
// seen: below 0 when no scan has ended.
inline int64_t tail_seen( int64_t seen, int64_t count )
{
	return std::max<int64_t>( count, seen < 0 ? 0 : seen / 2 );
}

// count_max: tail_seen() over the scans this scanner has ended, below 0 when it has ended none
inline TailPlan plan_tail( int64_t count_max, int64_t hit_cap, const TailOpts &o )
{
	TailPlan	p;
	if( o.spec_tail == 0 || o.dbg != 0 || o.timing != 0 || o.host_sort != 0 || o.timed_apart )
		return p;
	if( count_max < 0 || hit_cap < 2 )
		return p;
	// a quarter above what the scans before had (tail_seen): a steady sequence of scans is planned alike
	p.n_sort = std::min<int64_t>( hit_cap, std::max<int64_t>( RMA_TAIL_MIN, count_max + count_max / 4 ) );
	p.speculate = true;
	return p;
}

// what search_finish() repeats a launch for, as the counters of the launch say it
struct TailRepeat {
	bool	queue_need = false;		// general instance: a tile's items beyond queue and spill area
	bool	flush_queue_need = false;	// the instance that walks nothing: the same
	bool	list_need = false;		// ... and items beyond the end of the drain kernel's list
	bool	piece_overflow = false;		// a piece of an item beyond its order words, and the scanner not yet on whole items
	bool	any() const { return queue_need || flush_queue_need || list_need || piece_overflow; }
};

enum TailVerdict : int { TAIL_REDO = 0, TAIL_TAKE = 1 };

// count: RMK_C_COUNT as the kernels left it; flag: the ordering found a header word beyond its key; n: the records the
// scan ends with (the count, where nothing is repeated).  No records and one record keep their own ways out.
inline TailVerdict tail_verdict( unsigned long long count, int64_t n_sort, int64_t hit_cap, const TailRepeat &r, bool flag, int64_t n )
{
	if( r.any() || flag )
		return TAIL_REDO;
	if( hit_cap < 0 || n_sort < 0 || count > ( unsigned long long )hit_cap || count > ( unsigned long long )n_sort )
		return TAIL_REDO;
	if( n < 2 || ( unsigned long long )n != count )
		return TAIL_REDO;
	return TAIL_TAKE;
}

}	// namespace rma
