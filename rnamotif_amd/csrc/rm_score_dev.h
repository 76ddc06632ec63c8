// rm_score_dev.h -- the score section's MAIN program over hit records on the device (rma_score_hits, rm_hitpost.cpp).
// The rule -- every instruction, every stop -- is rm_score_core.h's, shared with the host; the image it runs is
// rm_score_image.h's.
//
//   rma_score_kernel   one record per lane.  A workgroup of 1 to 4 waves copies the image into LDS once, makes the two
//                      letter tables of rm_hitwin_dev.hip's gather kernel (byte -> letter, byte -> complement) next to
//                      it, and gives every wave its planes: slot k of lane l at word k * 64 + l, three words a stack
//                      slot or variable, then a byte a slot of the element stack.  All of a lane's runtime-indexed
//                      state is there; the wave's access to one slot touches 64 consecutive words.  A lane checks its
//                      record by the replay's rule (hitwin_span, rm_hitwin.h) before it reads anything the record
//                      points to -- a bad record's index goes into *bad by an atomic minimum and nothing is run for it --
//                      and reads bases from the database's text through the accessor: table, strand-1 complement, 'n'
//                      outside the entry.  A stopped record's index goes into *stopped the same way.
//                      The dynamic LDS is sized at launch: the image, 512 bytes of tables, waves * rms_wave_bytes().
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "rm_hitwin.h"
#include "rm_score_image.h"

struct RmsResult;
namespace rma {

struct ScoreBatch {
	const void	*image;		// the first `bytes` bytes of an image, in device memory
	int32_t	image_bytes, stack, n_vars;
	const int32_t	*hits;
	long long	n, first;	// records of this launch; the index of the first among the call's
	int32_t	stride;
	HitWinShape	shape;
	const int32_t	*slen;
	const int64_t	*start;
	int32_t	n_seq;
	const uint8_t	*text, *table;
	int32_t	codes;			// the table holds codes of the database's alphabet, not letters
	int32_t	budget;
	uint8_t	*accept;		// [ n ] 1 accepted, 0 rejected (or bad, or stopped)
	double	*score;			// [ n ]
	int8_t	*kind;			// [ n ]
	unsigned long long	*bad, *stopped;	// the least index of a bad / a stopped record, preset to ~0
	RmsResult	*detail;		// not null: where a stopped record leaves its result (a launch of one record)
};

#if defined( __HIPCC__ )
// the letters Replay.device() reads: the table's (of a code: its letter), on strand 1 the complement, read downwards
// (rma_score_kernel and rma_seqcheck_kernel of rm_seqcheck_dev.hip read bases through it)
struct ScoreBases {
	const uint8_t	*text;		// the entry's first byte
	const uint8_t	*let, *cmp;	// in LDS
	int	comp, slen;
	__device__ unsigned char	operator()( int i ) const
	{
		if( unsigned( i ) >= unsigned( slen ) )
			return 'n';
		return comp ? cmp[ text[ slen - 1 - i ] ] : let[ text[ i ] ];
	}
};
#endif

// waves of a workgroup: as many of 4 as RMS_LDS_BYTES hold next to the image (0: not one)
int	score_waves( int image_bytes, int stack, int n_vars );
// Enqueue on s the rule over the batch's records.
hipError_t	score_records( const ScoreBatch &b, hipStream_t s );
// the kernel's private bytes, static LDS and registers as the runtime reports them (rma_score_info)
hipError_t	score_kernel_attributes( int *private_bytes, int *static_lds, int *regs );

}	// namespace rma
