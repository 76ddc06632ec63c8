// rm_launch_plan.h -- the launch shape of a scan, chosen on the host without a HIP call: the tile sizes of a
// descriptor, the layout of a database (tile size, groups, tiles over the concatenation, the instance that walks
// nothing), its tiling, and per scan the kernel instance, grid, LDS and the drain kernel's shape.  rm_scanner.cpp
// owns the resources and calls these; tests/test_launch_plan.py pins them on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "rm_kernels.h"
#include "rnamotif_amd_program.h"

namespace rma {

// launch-shape and diagnostic switches: read from the environment once, when the scanner is
// created (DESIGN.md has the table), changed afterwards only through rma_scanner_set_option()
struct Options {
	int	dbg = 0;
	int	pool = -1;		// -1: by the descriptor, 0: pass B tile by tile
	int	pool_min = 1024, pool_refill = 48;
	int	drain = 1;		// pooled instance: the items are walked by a kernel of their own (0: by the workgroup that found them)
	int	glist = 0;		// > 0: items of the drain kernel's list (tests: a list that overflows), 0: by the database's size
	int	drain_waves = 6;	// workgroups (of one wave) of the drain kernel per CU; 0: what LDS and registers allow (16).  Six: the kernel alone
				// is as fast as with 16 (profiles/overlap_try.py: 0.29 ms).  (Five search workgroups a CU leave a SIMD 72 registers and
				// this kernel needs 128: it starts beside another scanner's search kernel only under a plan made for that -- `beside`)
	int	flush = -1;		// pooled instance that walks nothing (RMK_LEAN_FLUSH): -1 where the descriptor has a look-ahead chain, 0 never, 1 wherever the pooled instance runs
	int	efn_light = -1;		// the energy kernel in workgroups of one wave that stage no tables (rma_efn_light_kernel): -1 by the scan's instance, 0 never, 1 always
	int	search_wgs = 0;		// > 0: workgroups of a lean search kernel per CU (fewer than fit: another scanner's drain kernel runs beside it)
	int	beside = -1;		// the instance that walks nothing, planned so that another scanner's drain kernel is sure of room beside it (plan_beside):
				// -1 when another scanner of the device has a scan in flight (rma_scan_begin resolves it), 0 never, 1 always; plan_launch reads 1 as on
	int	struct_wgs = 0;		// > 0: workgroups of the kernels of rma_structure_energies (tests: a grid-stride loop over a few hundred structures)
	int	score_budget = 1 << 20;	// instructions of the score section a record of rma_score_hits may take before it stops (RMS_DEFAULT_BUDGET)
	int	score_heap = 256;	// bytes of heap a record of a score program with text has for the strings it makes (RMS_DEFAULT_HEAP)
	int	host_sort = 0, timing = 0;
	int	spec_tail = -1;		// a scan's tail enqueued by rma_scan_begin, ahead of the count (rm_tail_plan.h): -1 by the rule, 0 never
	int	short_force = -1;	// -1: by the mean entry length, 0 never, 1 always groups of small tiles, 2 always tiles over the concatenation
	int	tile = 0, qcap = 0;	// forced tile size / queue entries, 0: computed
	int	spill = -1;		// forced spill area, -1: SPILL_ITEMS
	int	budget = 0;
	void	latch();
	bool	set( const std::string &name, int value );	// an option that may change after creation (false: no such option)
};

// LDS of one search workgroup: program image | queue | tile | 6 bit vectors | lean records
size_t	search_lds_bytes( int prog_bytes, const rmd_program_t &dp, int tile_t, bool lean, int qcap, int group = 1, bool flush = false );

// what rma_scanner_create sizes once per descriptor
struct ProgramPlan {
	const rmd_program_t	*dp = nullptr;
	int	prog_bytes = 0, strands = 1, dminlen = 0;
	int	kinds = 0;			// RMD_KIND_* of the descriptor
	int	tile_t = 2048, qcap = QCAP;	// the tile and work queue of the one-tile instances
	bool	flush = false;			// the instance that walks nothing can run, on tiles of its own size
	int	tile_t_flush = 0, qcap_flush = 0;
};
ProgramPlan	plan_program( const rma_program_t &prog, const rmd_program_t &dp, int prog_bytes, int spill_cap, const Options &o );
// workgroups of a general instance where one of a lean instance stands (1 for lean descriptors)
inline int	wgs_per_wave( const rmd_program_t &dp ) { return dp.lean_ok ? 1 : SEARCH_BLOCK / GENERAL_BLOCK; }

// what the layout of a database depends on
struct DbShape {
	int32_t	n_seq = 0;
	int64_t	sum_slen = 0, padded_bases = 0;
	bool	ranges = false, ascending = true;
};

// the launch shape a tiling is made for (rma_db keeps one tiling per key)
struct LayoutKey {
	int	tile_t = 0, dminlen = 0, strands = 0, group = 1, qcap = 0;
	bool	flush = false;		// tiles of the size of the pooled instance that walks nothing (RMK_LEAN_FLUSH)
	// Tiles over the CONCATENATION of the entries (round 4; databases of short entries, pooled lean instance): a
	// strand of the whole packed array -- the entries one after the other, each padded to 32 bases -- is tiled as
	// if it were one long entry, so that the vectors of a tile are full whatever the entries' lengths; what a
	// tile's tests let through is brought back to its entry when it enters the pool (super_convert in the kernel).
	bool	concat = false;
	bool	operator==( const LayoutKey &o ) const
	{
		return tile_t == o.tile_t && dminlen == o.dminlen && strands == o.strands && group == o.group && qcap == o.qcap &&
			concat == o.concat && flush == o.flush;
	}
};
LayoutKey	choose_layout( const ProgramPlan &pp, const Options &o, const DbShape &db, int cus );

// the tiling of a database for one key, on the host
struct Tiling {
	int64_t	n_tiles = 0;
	int64_t	concat_bases = 0;
	std::vector<int64_t>	h_tile_start;	// [n_seq + 1] prefix sum of tiles over the entries
	std::vector<int32_t>	h_tile_seq;	// [n_tiles] entry of every tile
	// one tile per workgroup pass: all a workgroup needs to know of tile t in one 32-byte line (RMK_META_*), so that it
	// is one load -- made a tile ahead, straight into LDS -- instead of three dependent ones at the tile's start
	std::vector<int32_t>	h_tile_meta;
};
void	make_tiling( const LayoutKey &k, const std::vector<int32_t> &slen, const std::vector<int64_t> &base_off,
		const std::vector<int32_t> &pos_lo, const std::vector<int32_t> &pos_hi, int64_t padded_bases, Tiling *out );

// the launch of one scan
struct LaunchPlan {
	bool	lean = false, grouped = false, pooled = false;
	int	inst = 0, grid = 0, tile_bytes = 0;
	size_t	lds = 0;
	int	drain_nib = 0, drain_grid = 0;	// (pooled instances only)
	size_t	drain_lds = 0;
	bool	listed = false;		// the instance hands items to the drain kernel's list
	bool	walks_nothing = false;	// ... all of them (RMK_LEAN_FLUSH, RMK_LEAN_CONCAT_FLUSH)
	bool	efn_light = false;	// the energy kernel behind it is rma_efn_light_kernel
	bool	beside = false;		// grid, lds and drain_grid leave another scanner's drain kernel room on every CU (option beside)
};
// 1 and err: the scan cannot be launched
int	plan_launch( const LayoutKey &k, int64_t n_tiles, const ProgramPlan &pp, const Options &o, int cus, LaunchPlan *out,
		char *err, size_t errlen );

}	// namespace rma
