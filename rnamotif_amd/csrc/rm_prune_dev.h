// rm_prune_dev.h -- rmprune's rule over hit records on the device (rma_prune_hits, rm_hitpost.cpp): a keep flag per
// record.  The rule is rm_prune.h's, shared with the host.  No workgroup waits for another: every kernel reads what
// the one before it on the stream wrote.
//
//   rma_prune_keys_kernel     one lane per record: hitwin_span's checks (a failing record's index into *bad by an
//                             atomic minimum), then comp / start / stop as printed, the run-start flag (the name group
//                             of the record's entry differs from that of the record before it) and the ( start, stop )
//                             of every helix strand as locate() gives them into the record's key row -- a sequential
//                             walk over the printed fields, only helix strands written.  The workgroup's greatest
//                             run start goes into part[].
//   rma_prune_part_kernel     one workgroup: the exclusive scan of part[] (a maximum, later a sum), a lane walking a
//                             run of it, lane 0 the 256 runs.
//   rma_prune_starts_kernel   one lane per record: "the index of my run's first record" as a running maximum -- the
//                             workgroup's scan in LDS joined with what the workgroups before it have -- and from it
//                             the block-start flag: a block begins at every multiple of PRUNE_BLOCK from its run's
//                             start.  The workgroup's number of block starts goes into part[].
//   rma_prune_list_kernel     one lane per record: a block start writes its index into the list, at the place the
//                             scan of the counts gives it (whose total is the number of blocks).
//   rma_prune_rezip_kernel    one wave per block (a workgroup of 64, blocks taken grid-stride, so no launch bound).
//                             start / stop / comp and the keep flags of the block's records live in LDS (10 KB).
//                             first_comp by ballot; the leaders by repeated "first lane that leaves the leader's
//                             span" ballots over 64 records at a time; per group rezip(): for each kept b from the
//                             last down, the lanes take the b1 < b in descending chunks of 64 -- b's key row is
//                             wave-uniform, a lane reads its own b1's -- and ballot LEFT and DOWN among the kept
//                             ones: with a LEFT, the highest such b1 ends the pass, the DOWN lanes above it are
//                             dropped and b is dropped; otherwise the DOWN lanes are dropped and the next chunk
//                             follows.  That is the sequential loop's result exactly: inside one pass over b1 a keep
//                             flag changes only for a b1 that is not visited again.  keep[] goes out as bytes.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "rm_prune.h"

namespace rma {

constexpr int	PRUNE_WG = 256;		// records per workgroup of the per-record kernels

// the device memory of one call, all of it the scanner's scratch
struct PruneDev {
	const PruneTable	*tab;		// the program's table
	const int32_t	*groups;	// [ n_seq ] name group per entry, or null: the entry's index
	int32_t	*hdr;			// [ n ][ 4 ] comp, start, stop, run-start flag
	int32_t	*rows;			// [ n ][ row ] key rows
	uint8_t	*bflag;			// [ n ] block-start flags
	long long	*part, *part_x;	// [ parts ] a workgroup's summary / what the workgroups before it have
	long long	*blocks;	// [ <= n ] the block starts in ascending order
	unsigned long long	*bad;	// least index of a refused record, ~0: none
	long long	*n_blocks;
};

inline int64_t prune_parts( int64_t n ) { return ( n + PRUNE_WG - 1 ) / PRUNE_WG; }
inline int prune_row_words( const PruneTable &t ) { return 2 * ( t.n_slots > 0 ? t.n_slots : 1 ); }

// Enqueue on s: everything up to the list of blocks for the n > 0 records at d_hits; *d.bad (set to ~0 by the caller
// beforehand) and *d.n_blocks are what the host reads before it queues prune_rezip.
hipError_t	prune_blocks( const int32_t *d_hits, int64_t n, int stride, const HitWinShape &shape, int row, const int32_t *d_slen,
	int32_t n_seq, const PruneDev &d, hipStream_t s );

// Enqueue on s: keep[ n ] from the list of n_blocks blocks
hipError_t	prune_rezip( int64_t n, int row, const PruneDev &d, int64_t n_blocks, uint8_t *d_keep, hipStream_t s );

}	// namespace rma
