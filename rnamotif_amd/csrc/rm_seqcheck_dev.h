// rm_seqcheck_dev.h -- the loose seq= expressions over hit records on the device (rma_seqcheck_hits, rm_hitpost.cpp).
// The rule is rm_seqcheck.h's, shared with the host, and so is the image it runs.
//
//   rma_seqcheck_kernel   one record per lane, laid out as rma_score_kernel (rm_score_dev.h).  A workgroup of 1 to 4
//                         waves copies the image into LDS once, makes the two letter tables of rm_hitwin_dev.hip's
//                         gather kernel (byte -> letter, byte -> complement) next to it, and gives every wave its planes:
//                         slot k of lane l at word k * 64 + l -- nine bra and nine ket positions, then four words a
//                         frame of the matcher's stack.  All of a lane's runtime-indexed state is there, none in
//                         private memory; whatever slot each lane is at, the wave's access touches 64 different banks
//                         (lane l is always in bank l).  The workgroup copies its records' rows to the fixed rows with
//                         consecutive lanes on consecutive words.  Then a lane checks its record by the replay's rule
//                         (hitwin_span, rm_hitwin.h) before it reads anything the record points to -- a bad record's
//                         index goes into *bad by an atomic minimum and nothing is run for it -- and reads bases from the
//                         database's text through the score kernel's accessor: table, strand-1 complement.  A stopped
//                         record's index goes into *stopped the same way.
//                         The dynamic LDS is sized at launch: the image, 512 bytes of tables, waves * rmq_wave_bytes().
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "rm_hitwin.h"
#include "rm_seqcheck.h"

namespace rma {

struct SeqBatch {
	const void	*image;		// the first `bytes` bytes of an image, in device memory
	int32_t	image_bytes, frames;
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
	uint8_t	*keep;			// [ n ] 1 a candidate, 0 dropped (or bad, or stopped)
	int32_t	*fixed;			// [ n * stride ] the fixed rows, or null
	unsigned long long	*bad, *stopped;	// the least index of a bad / a stopped record, preset to ~0
	RmqResult	*detail;		// not null: where a stopped record leaves its result (a launch of one record)
};

// waves of a workgroup: as many of 4 as RMQ_LDS_BYTES hold next to the image (0: not one)
int	seqcheck_waves( int image_bytes, int frames );
// Enqueue on s the rule over the batch's records.
hipError_t	seqcheck_records( const SeqBatch &b, hipStream_t s );
// the kernel's private bytes, static LDS and registers as the runtime reports them (rma_seqcheck_info)
hipError_t	seqcheck_kernel_attributes( int *private_bytes, int *static_lds, int *regs );

}	// namespace rma
