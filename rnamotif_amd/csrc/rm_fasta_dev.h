// rm_fasta_dev.h -- FASTA text cut into entries in pieces that are looked at independently.
//
// One rule for the kernels of rm_fasta_dev.hip and the host (tests/hostsim/fasta_index_check.cpp):
// FastaStream::open() / parse() (rm_stream.cpp), which walk a file from its first byte, restated for
// chunks of FD_CHUNK bytes each of which is classified without knowing what came before it.
//
//   * An entry starts at a '>' that is not inside a definition line; the definition line runs from
//     there to the next '\n' (or the end of the text).  So the first '>' of a line starts an entry, a
//     later one on that line belongs to the definition, and a '>' in the middle of a line of letters
//     starts an entry too (FN_fgetseq ends a sequence at any '>', dbutil.c:104-121).
//   * An entry's letters are the bytes outside definition lines, up to the next start, for which
//     isalpha() holds in the "C" locale.  Everything else is dropped.
//   * What a chunk needs of the text before it is one bit: "inside a definition line".  A chunk's
//     effect on that bit, and its letters and starts for either value of it, is an FdSummary; the
//     summaries compose associatively (fd_compose), so the state, the letters and the entries before
//     every chunk come from a scan of the summaries.
#pragma once
#include <cstdint>

#if defined( __HIPCC__ )
#define FD_FN	__host__ __device__ inline
#else
#define FD_FN	inline
#endif

namespace rma {

// bytes of text per chunk: one workgroup of FD_THREADS lanes, each wave a quarter of it in dwords
constexpr int	FD_CHUNK = 16384;
constexpr int	FD_THREADS = 256;
// chunk summaries one workgroup scans; more chunks than this need the scan's second level
constexpr int	FD_SCAN_BLOCK = 256;
// bytes of a definition line ('>' included) that come to the host: just past the readers' 20000
constexpr int	FD_HEADER_CAP = 20000 + 256;

enum { FD_GT = 1, FD_NL = 2, FD_LETTER = 4 };

FD_FN unsigned fd_class( unsigned char b )
{
	if( b == '>' )
		return FD_GT;
	if( b == '\n' )
		return FD_NL;
	return ( ( b | 0x20u ) >= 'a' && ( b | 0x20u ) <= 'z' ) ? FD_LETTER : 0u;
}

// A run of bytes as a function of the state in front of it (0: outside, 1: inside a definition line).
template <typename Count>
struct FdSummaryT {
	Count	letters[ 2 ];	// letters the run adds to the clean text
	Count	starts[ 2 ];	// entries that start in it
	uint32_t	out;		// bit s: the state behind the run when s is the state in front of it
};
using FdSummary = FdSummaryT<uint32_t>;		// a chunk, a block of chunks
using FdSummary64 = FdSummaryT<int64_t>;	// a text

template <typename Count>
FD_FN FdSummaryT<Count> fd_identity()
{
	return FdSummaryT<Count>{ { 0, 0 }, { 0, 0 }, 2u };
}

// one byte
FD_FN FdSummary fd_byte( unsigned cls )
{
	if( cls & FD_GT )
		return FdSummary{ { 0, 0 }, { 1, 0 }, 3u };
	if( cls & FD_NL )
		return FdSummary{ { 0, 0 }, { 0, 0 }, 0u };
	return FdSummary{ { ( cls & FD_LETTER ) ? 1u : 0u, 0 }, { 0, 0 }, 2u };
}

// a, then b
template <typename CA, typename CB>
FD_FN FdSummaryT<CA> fd_compose( const FdSummaryT<CA> &a, const FdSummaryT<CB> &b )
{
	FdSummaryT<CA>	r;
	r.out = 0;
	for( int s = 0; s < 2; s++ ){
		const int	m = int( ( a.out >> s ) & 1u );
		// (selects, not indexed reads: the kernels keep summaries in registers)
		r.letters[ s ] = a.letters[ s ] + CA( m ? b.letters[ 1 ] : b.letters[ 0 ] );
		r.starts[ s ] = a.starts[ s ] + CA( m ? b.starts[ 1 ] : b.starts[ 0 ] );
		r.out |= ( ( b.out >> m ) & 1u ) << s;
	}
	return r;
}

// n bytes, one after the other
FD_FN FdSummary fd_summarise( const unsigned char *p, int64_t n )
{
	FdSummary	r = fd_identity<uint32_t>();
	for( int64_t i = 0; i < n; i++ )
		r = fd_compose( r, fd_byte( fd_class( p[ i ] ) ) );
	return r;
}

// What is in front of a chunk: the state, the letters and the entries started so far.
struct FdPrefix {
	int64_t	letters;
	int64_t	starts;
	int32_t	state;
	int32_t	pad_;
};

template <typename Count>
FD_FN FdPrefix fd_advance( const FdPrefix &p, const FdSummaryT<Count> &s )
{
	return FdPrefix{ p.letters + int64_t( p.state ? s.letters[ 1 ] : s.letters[ 0 ] ),
		p.starts + int64_t( p.state ? s.starts[ 1 ] : s.starts[ 0 ] ), int32_t( ( s.out >> p.state ) & 1u ), 0 };
}

// One byte with the state in front of it known: FD_LETTER kept, FD_GT an entry starts here, FD_NL a
// definition line ends here, 0 dropped.  *state is the state behind it.
FD_FN unsigned fd_apply_byte( unsigned cls, int *state )
{
	if( cls & FD_NL ){
		const unsigned	r = *state ? unsigned( FD_NL ) : 0u;
		*state = 0;
		return r;
	}
	if( *state )
		return 0u;
	if( cls & FD_GT ){
		*state = 1;
		return FD_GT;
	}
	return cls & FD_LETTER;
}

}	// namespace rma
