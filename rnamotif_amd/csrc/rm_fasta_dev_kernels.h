// rm_fasta_dev_kernels.h -- the entries and letters of FASTA text in HBM, found on the device
// (rma_db_create_device_fasta, rm_scanner.cpp).  The rule is rm_fasta_dev.h's, shared with the host.
//
//   rma_fasta_summarise_kernel    a workgroup per chunk of FD_CHUNK bytes: its FdSummary
//   rma_fasta_scan_blocks_kernel  a workgroup per FD_SCAN_BLOCK summaries: what lies before each chunk
//                                 inside its block (a summary), and the block's summary
//   rma_fasta_scan_top_kernel     one workgroup: what lies before each block, and the totals
//   rma_fasta_apply_kernel        a workgroup per chunk, its incoming state now known: the letters,
//                                 compacted, into the clean text; per entry the offset of its '>', of
//                                 the end of its definition line and of its first letter
//   rma_fasta_headers_kernel      a wave per entry: its definition line, capped, for the host
// No workgroup waits for another: each launch reads what the one before it wrote.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "rm_fasta_dev.h"

namespace rma {

inline int64_t fasta_chunks( const void *text, int64_t text_bytes )
{
	// (chunks are cut from the aligned dword the text begins in)
	const int64_t	v = int64_t( reinterpret_cast<uintptr_t>( text ) & 3u ) + text_bytes;
	return text_bytes > 0 ? ( v + FD_CHUNK - 1 ) / FD_CHUNK : 0;
}
inline int64_t fasta_blocks( int64_t chunks ) { return ( chunks + FD_SCAN_BLOCK - 1 ) / FD_SCAN_BLOCK; }

// Enqueue on s the first three kernels over text[ 0, text_bytes ), text_bytes > 0: d_sum and d_local hold
// fasta_chunks() summaries, d_block_sum fasta_blocks() summaries, d_block_pre as many prefixes; *d_totals is
// what lies behind the last byte.  Nothing outside the text's bytes is used (the aligned dwords its first and
// last bytes lie in are read whole).
hipError_t	fasta_index( const uint8_t *text, int64_t text_bytes, FdSummary *d_sum, FdSummary *d_local, FdSummary *d_block_sum,
	FdPrefix *d_block_pre, FdPrefix *d_totals, hipStream_t s );

// Enqueue on s, behind fasta_index(): clean[ 0, totals.letters ) and, for the totals.starts entries, gt_off / def_end
// (offsets from text; def_end is text_bytes for a last line without '\n') and first (offset in clean).
hipError_t	fasta_apply( const uint8_t *text, int64_t text_bytes, const FdSummary *d_local, const FdPrefix *d_block_pre,
	const FdPrefix *d_totals, uint8_t *clean, int64_t *d_gt_off, int64_t *d_def_end, int64_t *d_first, hipStream_t s );

// Enqueue on s: entry e's first min( def_end - gt_off, FD_HEADER_CAP ) bytes from its '>' to d_out + d_hdr_off[ e ]
hipError_t	fasta_headers( const uint8_t *text, int64_t text_bytes, const int64_t *d_gt_off, const int64_t *d_def_end,
	const int64_t *d_hdr_off, int64_t n, uint8_t *d_out, hipStream_t s );

}	// namespace rma
