// rm_structenergy_dev.h -- efn() and efn2() of structures in device tensors (rma_structure_energies, rm_hitpost.cpp).
// The rule -- what is refused, what is infinite, the candidate view of the cores -- is rm_structenergy.h's, shared with
// the host.
//
//   rma_struct_check_kernel    one wave per structure, grid-stride: the lanes take the structure's bases 64 at a time,
//                              each judges its base (rmse_check_base: the partner's range, symmetry, whether the base
//                              opens a helix, whether its pair crosses another or closes nothing), the wave adds up.  A
//                              refused structure's index goes into bad[ 0 ] by an atomic minimum; an accepted one's
//                              helix count and infinity flag into info[ s ]; bad[ 1 ] becomes 1 when some structure
//                              needs the instance with the large stacks.  Nothing else is written.
//   rma_struct_energy_kernel   the staged energy kernel's shape (rm_scan_kernel.h efn_body): workgroups of 256 lanes,
//                              efn's int16 table image staged once per workgroup into LDS, 16 bytes per lane and step,
//                              the 256 byte -> code table in LDS, one structure per lane in a grid-stride loop, the
//                              codes and partners of a structure of up to RMSE_CACHE bases in the lane's LDS rows,
//                              longer ones read from the tensors; efn2's tables in global memory.  Two instances: the
//                              usual stacks, and BIG for structures of more than RMSE_SMALL_HELICES helices; each
//                              takes the structures that info[] gives it and leaves the others alone, so a call is
//                              one launch, or two when bad[ 1 ] says so, with the same results either way.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "rnamotif_amd_program.h"

namespace rma {

struct StructBatch {
	const int64_t	*off;		// [ n + 1 ]
	const uint8_t	*base;		// [ total ]
	const int32_t	*pair;		// [ total ] every pair_stride words
	int32_t	pair_stride;
	int64_t	n, total;
};

// Enqueue on s the check of every structure: d_bad[ 0 ] (preset to ~0) the least index of a refused one, d_bad[ 1 ]
// (preset to 0) whether the BIG instance is needed, d_info[ n ].  wgs > 0: that many workgroups.
hipError_t	struct_check( const StructBatch &b, int32_t *d_info, unsigned long long *d_bad, int wgs, int cus, hipStream_t s );

struct StructTables {
	const int16_t	*t16;		// efn's tables (rma::efn_tables16), or null
	const int32_t	*tlkey, *loginc;
	const rma_efn2data_t	*e2;	// efn2's tables, or null
	const uint8_t	*code;		// [ 256 ] byte -> base code
};

// Enqueue on s the energies of the checked structures that take the instance `big` (0 / 1): d_efn[ s ] where d_efn and
// t16 are there, d_efn2[ s ] where d_efn2 and e2 are.  wgs > 0: that many workgroups, else one per CU at most.
hipError_t	struct_energies( const StructBatch &b, const int32_t *d_info, const StructTables &t, int32_t *d_efn, int32_t *d_efn2,
	int big, int wgs, int cus, hipStream_t s );

}	// namespace rma
