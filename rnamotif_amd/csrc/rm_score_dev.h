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
//   rma_score_text_kernel   the same for an image with RMS_IMG_TEXT or a call that wants the score column as bytes
//                      (rma_score_hits_text): the rule with its heap, sprintf(), bits() and the column's formatter.  A
//                      lane's heap is global memory of the scanner's, sized per launch: the 64 lanes of wave v (counted
//                      over the launch) own 64 * W dwords at v * 64 * W, W = ceil( heap_cap / 4 ); dword j of lane l is
//                      word j * 64 + l of them, so that the lanes of a wave writing the same offset of their strings
//                      touch 64 consecutive dwords.  The table of bits() stays in global memory.  A lane writes its
//                      row of the column itself; col_len[ h ] is the column's length, 0 for a record that is not accepted.
//                      rma_score_kernel is compiled from the rule without any of this (rms_run_t< false >).
//   rma_score_match_kernel, rma_score_match_text_kernel   the two above for an image with expressions (RMS_IMG_MATCH and
//                      a =~, a !~ or a mismatches( string, pattern ) in MAIN): score_body< TEXT, true >, the rule with
//                      do_mat and the builtin.  The expressions' ops come to LDS with the image.  A wave's planes are
//                      followed by its matcher's (rmq_wave_bytes( frames ), rm_seqcheck.h: 18 words of bra[] and ket[]
//                      and four words a frame, slot k of lane l at word k * 64 + l), so that the matcher's state, all of
//                      it indexed at run time, is in LDS like the rest and no lane has private memory for it.  Every
//                      other image runs the two kernels above, which are compiled from the rule without the matcher.
//   rma_score_text_copy_kernel   bytes [ 0, len[ h ] ) of every row from the scratch to the caller's rows: what lies
//                      behind a row's length is not written.
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
	// an image with RMS_IMG_TEXT, or a call with text outputs: rma_score_text_kernel
	int32_t	text_kernel = 0;
	uint8_t	*heap = nullptr;	// score_heap_bytes( n, heap_cap ) bytes of the scanner's
	int32_t	heap_cap = 0;		// bytes of heap a record has
	const double	*bits_tab = nullptr;	// the image's table of bits(), behind the image in device memory
	uint8_t	*col = nullptr;		// [ n, col_stride ] the score column, or null
	int32_t	col_stride = 0;
	int32_t	*col_len = nullptr;	// [ n ]
	// an image with expressions: rma_score_match_kernel / rma_score_match_text_kernel
	int32_t	match_kernel = 0;
	int32_t	frames = 0;		// of the matcher's planes (rms_frames())
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

// waves of a workgroup: as many of 4 as RMS_LDS_BYTES hold next to the image (0: not one); frames: of the matcher's planes
// behind each wave's own (rms_frames()), < 0 for an image without expressions
int	score_waves( int image_bytes, int stack, int n_vars, int frames = -1 );
// Enqueue on s the rule over the batch's records.
hipError_t	score_records( const ScoreBatch &b, hipStream_t s );
// the kernel's private bytes, static LDS and registers as the runtime reports them (rma_score_info); text: the text
// kernel's; match: the instance for an image with expressions
hipError_t	score_kernel_attributes( int *private_bytes, int *static_lds, int *regs, bool text = false, bool match = false );
// bytes of heap a launch of n records takes
size_t	score_heap_bytes( long long n, int heap_cap );
// Enqueue on s: bytes [ 0, len[ h ] ) of row h of src to row h of dst, n rows of `stride` bytes.
hipError_t	score_text_copy( uint8_t *dst, const uint8_t *src, const int32_t *len, long long n, int stride, hipStream_t s );

}	// namespace rma
