// rm_dbtext_dev.h -- the text of a packed database made on the device from its words in HBM (rm_dbtext.h has the rule).
//
// Three steps, enqueued one behind the other on one stream:
//  dbtext_directory	the rank directory: the mask bits of every run of 64 mask words counted, the counts scanned;
//  dbtext_check	per entry, the bases its mask has set against the number of its exceptions, and every exception
//			byte a letter the readers deliver at a masked position; the least bad entry through one word;
//			exc_base[] for the fill;
//  dbtext_fill		the text, a lane a slot of 16 bytes.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include "rm_dbtext.h"

namespace rma {

// Everything in device memory.  The database's words: codes[ 2 n_mask ], amask[ n_mask ], base_off[ n ], slen[ n ].
// exc[ n_exc ] and exc_off[ n + 1 ] (ascending from 0 to n_exc: the host has checked that), or exc null: a masked
// base reads n and nothing is counted against exc_off.  text_start[ n ] as rm_dbtext.h lays the text out, text_bytes
// its end.  Made here: dir[ runs ] with runs = dbtext_dir_runs( n_mask ) (counted, then scanned in place),
// exc_base[ n ], *bad, text[ text_bytes ] (16-byte aligned).
struct DbTextArgs {
	const uint32_t	*codes, *amask;
	long long	n_mask;
	const int64_t	*base_off;
	const int32_t	*slen;
	int32_t	n;
	const char	*exc;
	const int64_t	*exc_off;
	long long	n_exc;
	const int64_t	*text_start;
	long long	text_bytes;
	uint64_t	*dir;
	int64_t	*exc_base;
	unsigned long long	*bad;
	uint8_t	*text;
};

// (tmp null: *tmp_bytes becomes what the scan of the counts needs, nothing is enqueued)
hipError_t	dbtext_directory( const DbTextArgs &a, void *tmp, size_t *tmp_bytes, hipStream_t s );
// (*bad has been set to DT_BAD_NONE on s before)
hipError_t	dbtext_check( const DbTextArgs &a, hipStream_t s );
// hipErrorInvalidValue for a text of more slots than a grid has room for (2^40 bytes and more)
hipError_t	dbtext_fill( const DbTextArgs &a, hipStream_t s );

}	// namespace rma
