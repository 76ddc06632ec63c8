// rm_diag.h -- the two things the search and drain kernels (rm_scan_kernel.h) share with the host half of a
// scan (rm_scanner.cpp, rm_scan_report.cpp, rm_launch_plan.cpp) beyond their arguments: the bits of the `dbg`
// word (RNAMOTIF_DBG, option "dbg") and the slots of the counter block behind a launch.  Plain enums only, no
// HIP: host modules and CPU tests include it.  rnamotif_amd/__init__.py (DBG) and DESIGN.md's table of
// switches repeat the bits; tests/test_diag_names.py holds the three together and pins the slots.
#pragma once

// ---------------------------------------------------------------- the dbg word
// None of the bits changes the output of a scan that runs to its end (the ablation switches that cut the
// kernel short leave candidates out; they are for timing).  The values are what users set RNAMOTIF_DBG to.
enum rmk_dbg : int {
	// ---- path selectors: the tests force code paths with these
	RMK_DBG_GENERAL		= 16,		// the general instance for lean descriptors
	RMK_DBG_POOL_DROP	= 2048,		// the pooled instance fills the pool and drops it (no list, no drain kernel)
	RMK_DBG_WHOLE_ITEMS	= 2097152,	// items go whole into the drain kernel's list, not cut into pieces (the host sets it itself: RMK_C_PIECE_OVERFLOW)
	RMK_DBG_NO_FORKS	= 4194304,	// drain kernel: no subtrees handed to idle lanes
	RMK_DBG_LIST_ALL	= 8388608,	// everything a workgroup holds at the end goes to the list, not only fewer than GLIST_BELOW items

	// ---- ablation switches: a stage or a filter off, for what it costs or saves
	RMK_DBG_NO_PASS_B	= 1,		// pass B is skipped: the pre-filter alone (bench.py)
	RMK_DBG_NO_BITPAR	= 4,		// no bit-parallel pre-filter
	RMK_DBG_NO_LITERAL	= 8,		// no literal filter
	RMK_DBG_NO_ROWS		= 64,		// general instance: no pair rows in the search, end by end
	RMK_DBG_NO_VOTE		= 128,		// general instance: no level voting, every lane's level gets its round
	RMK_DBG_NO_SPLIT	= 256,		// general instance: no continuations
	RMK_DBG_NO_STEP_CHAIN	= 512,		// general instance: a step is one transition, it does not go on across levels (rmd_gen_step: chain)
	RMK_DBG_NO_HEAD_TEST	= 4096,		// pooled instance: no head-helix test in pass A'
	RMK_DBG_NO_Q1_FILTER	= 8192,		// no strand filter of a leading 4-plex
	RMK_DBG_NO_TRI_FILTER	= 16384,	// ... nor of the triplex behind it
	RMK_DBG_NO_CHAIN	= 32768,	// no look-ahead chain
	RMK_DBG_STOP_ROWS	= 65536,	// the kernel stops after decode and rows; nothing is queued
	RMK_DBG_STOP_CHAIN	= 131072,	// ... after the look-ahead chain; nothing is queued
	RMK_DBG_NO_HEAD_NEXT	= 262144,	// pass A': no joint D-arm / next-leaf test (it is off without the chain, too)
	RMK_DBG_NO_START_VEC	= 33554432,	// pass A goes position by position, not over the words of a vector of start positions worth a look (best literal / 4-plex' second strand within reach)
	RMK_DBG_TICKET_PER_TILE	= 67108864,	// a ticket per tile instead of one per TICKET_TILES tiles
	RMK_DBG_HEAD_ALL_ENDS	= 134217728,	// pass A' leaves the first interior helix every end its own length allows
	RMK_DBG_DRAIN_DROP	= 268435456,	// the drain kernel lays out its items' windows and drops them

	// ---- instrumentation: counters the host prints as [dbg] lines (rm_scan_report.cpp)
	RMK_DBG_COUNT_QUEUED	= 2,		// count queued items
	RMK_DBG_CYCLES		= 32,		// wave cycles per phase, wave rounds / lanes per search level (lean: pop rounds and steps with their lanes; drain kernel: its items and laps)
	RMK_DBG_TIMELINE	= 1048576,	// workgroup timeline of the search kernel
	RMK_DBG_DRAIN_DONE	= 536870912	// when the drain kernel's waves are through, in bins of 16 us
};

// ---------------------------------------------------------------- the counter block
// RMK_N_COUNTERS 64-bit words, zeroed before every launch; RMK_C_* is a word's index from its start
// (rma_scanner::d_counters, HitBuf::count; HitBuf::ticket points at word 1).  Diagnostic slots mean what the
// kernel that wrote them says: the general instances, the lean search instances and the drain kernel each
// have their names below, some with the same value.  The drain kernel runs behind a lean search kernel on the
// same block: RMK_C_EMITTED / RMK_C_DRAIN_LANES gets both kernels' sums when both walk items.
#define RMK_N_COUNTERS		128
#define RMK_GCTL		100		// the drain kernel's list: RMK_C_LIST_*
// how many words a binned range has: names of their own (RMK_CN_*), so that an extent is not taken for a slot
enum rmk_extent : int {
	RMK_CN_PHASES		= 6,		// RMK_C_PHASE
	RMK_CN_GEN_LEVELS	= 32,		// RMK_C_GEN_LEVEL, two words a level
	RMK_CN_LOG2_BINS	= 32,		// RMK_C_STEP_LOG2, RMK_C_DRAIN_LOG2, RMK_C_DRAIN_DONE
	RMK_CN_LEVEL_BINS	= 16,		// RMK_C_LEVEL_CYCLES, RMK_C_LEVEL_STEPS
	RMK_CN_EMIT_BINS	= 16,		// RMK_C_DRAIN_EMIT_ITEMS, RMK_C_DRAIN_EMIT_CYCLES
	RMK_CN_DRAIN_LAPS	= 4		// RMK_C_DRAIN_LAP
};
enum rmk_counter : int {
	RMK_C_COUNT		= 0,		// candidates found (may exceed HitBuf::cap)
	RMK_C_TICKET		= 1,		// next tile
	RMK_C_QUEUED		= 2,		// RMK_DBG_COUNT_QUEUED: items queued, all tiles
	RMK_C_QUEUE_NEED	= 3,		// general instances: most items of a tile, when more than queue and spill area hold (the host repeats the launch)
	RMK_C_PIECE_OVERFLOW	= 3,		// lean instances, drain kernel: a piece of an item found more candidates than PIECE_ORDER_BITS leave room for (... with whole items)
	RMK_C_PHASE		= 4,		// RMK_DBG_CYCLES, search kernel: wave cycles of RMK_CN_PHASES phases -- decode, literal, rows, pre-filter, search, waiting

	// RMK_DBG_CYCLES, general instances: per search level, wave rounds and the lanes served
	RMK_C_GEN_LEVEL		= 16,		// [RMK_CN_GEN_LEVELS][2]

	// RMK_DBG_CYCLES, lean search instances (pass B tile by tile writes the first six)
	RMK_C_POP_ROUNDS	= 16,
	RMK_C_POP_LANES		= 17,
	RMK_C_STEPS		= 18,
	RMK_C_STEP_LANES	= 19,
	RMK_C_POP_CYCLES	= 20,
	RMK_C_STEP_CYCLES	= 21,
	RMK_C_STEP_LONGEST	= 22,		// cycles of the longest single step
	RMK_C_WAVE_MOST		= 23,		// the most cycles any wave spent stepping in one session
	RMK_C_STEP_LOG2		= 24,		// [RMK_CN_LOG2_BINS] steps by log2( cycles )
	RMK_C_LEVEL_CYCLES	= 61,		// [RMK_CN_LEVEL_BINS] step cycles by deepest level
	RMK_C_LEVEL_STEPS	= 77,		// [RMK_CN_LEVEL_BINS] steps by deepest level
	RMK_C_EMIT_CYCLES	= 93,		// cycles storing complete matches
	RMK_C_EMITTED		= 94,		// complete matches

	// RMK_DBG_TIMELINE, search kernel (100 MHz clock; printed for the lean instances); they lie over the last
	// RMK_C_LEVEL_STEPS bins and the general instances' last levels, so the two bits are not set together
	RMK_C_TL_WGS		= 88,		// workgroups that had tiles
	RMK_C_TL_START		= 89,		// ~( the first workgroup's start )
	RMK_C_TL_DRY_SUM	= 90,		// sum of the times they ran out of tiles
	RMK_C_TL_DONE_MAX	= 91,		// the last to be done
	RMK_C_TL_DONE_SUM	= 92,

	// RMK_DBG_CYCLES, drain kernel
	RMK_C_DRAIN_ITEMS	= 18,		// items walked
	RMK_C_DRAIN_STEPS	= 19,
	RMK_C_DRAIN_CYCLES	= 21,
	RMK_C_DRAIN_LONGEST	= 22,		// cycles of the longest item
	RMK_C_DRAIN_MOST_STEPS	= 23,
	RMK_C_DRAIN_LOG2	= 24,		// [RMK_CN_LOG2_BINS] items by log2( cycles )
	RMK_C_DRAIN_EMIT_ITEMS	= 61,		// [RMK_CN_EMIT_BINS] items by complete matches: 0, 1, 2-3, 4-7, ...
	RMK_C_DRAIN_EMIT_CYCLES	= 77,		// [RMK_CN_EMIT_BINS] ... and their cycles
	RMK_C_DRAIN_LANES	= 94,		// busy lanes, summed over the wave rounds
	RMK_C_DRAIN_LAP		= 95,		// [RMK_CN_DRAIN_LAPS] wave cycles taking items, stepping, storing complete matches, handing over
	RMK_C_DRAIN_ROUNDS	= 99,		// wave rounds

	// RMK_DBG_DRAIN_DONE, drain kernel; the bins are RMK_C_DRAIN_LOG2's words, so not together with RMK_DBG_CYCLES
	RMK_C_DRAIN_DONE	= 24,		// [RMK_CN_LOG2_BINS] waves through by 16 us from ...
	RMK_C_DRAIN_START	= 56,		// ~( the first wave's start )

	// the drain kernel's list and the instance that walks nothing (no diagnostics: the host reads them after every launch)
	RMK_C_LIST_RESERVED	= RMK_GCTL,	// items reserved in the list (may exceed HitBuf::glist_cap: the host repeats the scan with a longer one)
	RMK_C_LIST_TAKEN	= RMK_GCTL + 1,	// ... and taken by the drain kernel
	RMK_C_FLUSH_QUEUE_NEED	= RMK_GCTL + 2,	// the instance that walks nothing: RMK_C_QUEUE_NEED's counterpart
	RMK_C_COPIED		= RMK_GCTL + 3	// words the host copies back after every launch
};

// what one kernel writes under one instrumentation bit does not overlap and stays inside the block
static_assert( RMK_C_PHASE > RMK_C_QUEUE_NEED && RMK_C_PHASE + RMK_CN_PHASES <= RMK_C_GEN_LEVEL, "phases" );
static_assert( RMK_C_GEN_LEVEL + 2 * RMK_CN_GEN_LEVELS <= RMK_C_LIST_RESERVED, "general instances: levels" );
static_assert( RMK_C_WAVE_MOST < RMK_C_STEP_LOG2 && RMK_C_STEP_LOG2 + RMK_CN_LOG2_BINS <= RMK_C_LEVEL_CYCLES &&
	RMK_C_LEVEL_CYCLES + RMK_CN_LEVEL_BINS <= RMK_C_LEVEL_STEPS && RMK_C_LEVEL_STEPS + RMK_CN_LEVEL_BINS <= RMK_C_EMIT_CYCLES &&
	RMK_C_EMITTED < RMK_C_LIST_RESERVED, "lean instances: pass B" );
static_assert( RMK_C_TL_WGS > RMK_C_PHASE + RMK_CN_PHASES && RMK_C_TL_DONE_SUM < RMK_C_LIST_RESERVED, "lean instances: timeline" );
static_assert( RMK_C_DRAIN_MOST_STEPS < RMK_C_DRAIN_LOG2 && RMK_C_DRAIN_LOG2 + RMK_CN_LOG2_BINS <= RMK_C_DRAIN_EMIT_ITEMS &&
	RMK_C_DRAIN_EMIT_ITEMS + RMK_CN_EMIT_BINS <= RMK_C_DRAIN_EMIT_CYCLES && RMK_C_DRAIN_EMIT_CYCLES + RMK_CN_EMIT_BINS <= RMK_C_DRAIN_LANES &&
	RMK_C_DRAIN_LANES < RMK_C_DRAIN_LAP && RMK_C_DRAIN_LAP + RMK_CN_DRAIN_LAPS <= RMK_C_DRAIN_ROUNDS && RMK_C_DRAIN_ROUNDS < RMK_C_LIST_RESERVED, "drain kernel: items and laps" );
static_assert( RMK_C_DRAIN_DONE + RMK_CN_LOG2_BINS <= RMK_C_DRAIN_START && RMK_C_DRAIN_START < RMK_C_LIST_RESERVED, "drain kernel: waves through" );
static_assert( RMK_C_COPIED <= RMK_N_COUNTERS, "the block" );
