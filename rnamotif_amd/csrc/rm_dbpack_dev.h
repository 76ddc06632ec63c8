// rm_dbpack_dev.h -- a database's packed words made on the device from text already in HBM.
//
// The same words rma::PackedDb::add() (rm_fasta.cpp) makes on the host: entry i at base_off[i] (a
// multiple of 32, entries one after the other), per 32 bases one ambiguity mask word and two code words,
// every bit past an entry's last base zero.  Entry i's text is the slen[i] bytes at text + start[i]; a
// byte becomes table[ byte ] (0-3 a code, anything above 3 ambiguous: code 0, mask bit set).
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>

namespace rma {

// Enqueue on s: codes[ 0, 2 * mask_words ) and amask[ 0, mask_words ), every word written.  d_start,
// d_base_off, d_slen hold n entries and d_table 256 bytes, all in device memory (4-byte aligned table);
// the caller has checked that every entry's bytes lie inside the text's allocation.
hipError_t	pack_text( const uint8_t *text, const int64_t *d_start, const int64_t *d_base_off, const int32_t *d_slen, int32_t n,
	int64_t mask_words, const uint8_t *d_table, uint32_t *codes, uint32_t *amask, hipStream_t s );

}	// namespace rma
