// rm_scan_report.h -- the [dbg] lines of a scan (option "dbg", RNAMOTIF_DBG): what the kernels left in the
// counter block (rm_diag.h), printed to stderr.  No HIP: the scanner hands over a host copy of the block.
#pragma once
#include <cstddef>
#include "rm_dev_program.h"
#include "rm_diag.h"

namespace rma {

// what the report says of the launch, and what decides which kernel's names the slots go by
struct ScanShape {
	int	dbg;
	int	tile_t, group, qcap, grid;	// (group: tiles per workgroup pass, 1 unless grouped)
	size_t	lds;
	long long	n_tiles;
	bool	lean;			// a lean search instance ran
	bool	drained;		// ... and the drain kernel behind it
};

// ctr: all RMK_N_COUNTERS words as the launch left them
void	debug_report( const unsigned long long *ctr, const ScanShape &s, const rmd_program_t &dp );

}	// namespace rma
