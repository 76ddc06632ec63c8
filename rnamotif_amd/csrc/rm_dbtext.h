// rm_dbtext.h -- the text of a packed database: one byte per base, made from its 2-bit code words, its mask words
// and the letters at the masked positions.
//
// One rule for the host (tests/hostsim/dbtext_check.cpp, which holds it to PackFile::unpack) and the device (the
// kernels of rm_dbtext_dev.hip).  Entry e of a database has its code words at base_off / 16, its mask words at
// base_off / 32 (base_off is a multiple of 32), slen bases, and in exc[] the letters at its masked positions in
// order, from exc_off[ e ] on.  Base p of it reads
//	"acgt"[ code ]			where its mask bit is clear,
//	exc[ exc_off[ e ] + rank( p ) ]	where it is set, rank( p ) the mask bits set below p within the entry,
//	n				where it is set and there are no exceptions.
// Mask bits at or above slen in the entry's last word are padding: they lie above every base of the entry and are
// never counted for one.  Word and exception indices are 64-bit (base_off passes 2^32, exc_off can); a position
// within an entry is an int32_t.
//
// The text: entry e's bytes begin at text_start[ e ], a multiple of 16 -- the entries one after the other, each
// rounded up to whole slots of 16 bytes, the bytes past slen in an entry's last slot n.  Slot t of the text (bytes
// [ 16 t, 16 t + 16 )) is one code word of one entry: the unit of the fill.
//
// Ranks come from a sparse directory over the database's mask words, whatever order its entries lie in: dir[ r ] is
// the number of mask bits set in words [ 0, 64 r ) -- one count per run of DT_RUN_WORDS mask words, 8 bytes per
// 2048 bases.  G( W ) = dir[ W / 64 ] + the bits of words [ W & ~63, W ) counts the bits below word W; the words of
// one entry are consecutive, so G( W ) - G( base_off / 32 ) is the rank of the first base of word W of the entry
// and exc_base = exc_off[ e ] - G( base_off / 32 ) turns any G into an index into exc[].
#pragma once
#include <cstddef>
#include <cstdint>

#if defined( __HIPCC__ )
#define RMT_FN	__host__ __device__ inline
#else
#define RMT_FN	inline
#endif

namespace rma {

constexpr int	DT_SLOT = 16;			// bases of a code word: bytes of a slot of the text
constexpr int	DT_RUN_WORDS = 64;		// mask words of a run of the directory (2048 bases)

// ---- where things are (64-bit throughout)
RMT_FN int64_t dbtext_code_word( int64_t base_off, int32_t p ) { return base_off / 16 + ( p >> 4 ); }
RMT_FN int64_t dbtext_mask_word( int64_t base_off, int32_t p ) { return base_off / 32 + ( p >> 5 ); }
RMT_FN int64_t dbtext_run( int64_t mask_word ) { return mask_word / DT_RUN_WORDS; }
RMT_FN int64_t dbtext_run_first( int64_t mask_word ) { return mask_word - mask_word % DT_RUN_WORDS; }
// bytes of an entry in the text; runs of a directory over n_mask words (one more than the words need: G( n_mask ))
RMT_FN int64_t dbtext_entry_bytes( int32_t slen ) { return ( int64_t( slen ) + DT_SLOT - 1 ) / DT_SLOT * DT_SLOT; }
RMT_FN int64_t dbtext_dir_runs( int64_t n_mask ) { return n_mask / DT_RUN_WORDS + 1; }
// the index into exc[] of a masked base: the entry's exc_base, the directory's count for the run of the base's mask
// word, the bits of the run's words before that word, the bits of that word below the base
RMT_FN int64_t dbtext_exc_index( int64_t exc_base, int64_t dir_run, int64_t in_run, int below ) { return exc_base + dir_run + in_run + below; }

RMT_FN int dbtext_popcount( uint32_t x )
{
#if defined( __HIP_DEVICE_COMPILE__ )
	return __popc( x );
#else
	return __builtin_popcount( x );
#endif
}

// the mask bits of slot `cw` (a code word's number within the entry) of an entry of slen bases: bit j is base
// 16 cw + j; only bases of the entry (bits at or above slen are padding)
RMT_FN uint32_t dbtext_slot_mask( uint32_t mask_word, int64_t cw, int32_t slen )
{
	const uint32_t	half = ( cw & 1 ) ? mask_word >> 16 : mask_word & 0xffffu;
	const int64_t	left = int64_t( slen ) - 16 * cw;
	return left >= 16 ? half : left <= 0 ? 0u : half & ( ( 1u << int( left ) ) - 1u );
}
// ... and the bits of the slot that are no bases at all (the tail of the entry's last slot)
RMT_FN uint32_t dbtext_slot_tail( int64_t cw, int32_t slen )
{
	const int64_t	left = int64_t( slen ) - 16 * cw;
	return left >= 16 ? 0u : left <= 0 ? 0xffffu : 0xffffu & ~( ( 1u << int( left ) ) - 1u );
}
// the mask bits of a mask word below bit b (0-31) that slot counts ahead of itself: the lower half for an odd slot
RMT_FN uint32_t dbtext_below_slot( uint32_t mask_word, int64_t cw ) { return ( cw & 1 ) ? mask_word & 0xffffu : 0u; }
// the bits of the entry's word `w` (0: its first) that are bases of it
RMT_FN uint32_t dbtext_word_bases( uint32_t mask_word, int64_t w, int32_t slen )
{
	const int64_t	left = int64_t( slen ) - 32 * w;
	return left >= 32 ? mask_word : left <= 0 ? 0u : mask_word & ( ( 1u << int( left ) ) - 1u );
}

// a letter the readers deliver at a masked position: lower case, not a, c, g or t (u has become t)
RMT_FN bool dbtext_exc_letter( unsigned char b ) { return b >= 'a' && b <= 'z' && b != 'a' && b != 'c' && b != 'g' && b != 't'; }

// eight 2-bit codes (the low 16 bits of x) as eight letters, one a byte, the first code the lowest: the codes
// spread to a byte each, then a + 2 b0 + 6 b1 + 11 b0 b1 of a code's two bits -- a, c, g, t
RMT_FN uint64_t dbtext_letters8( uint32_t x )
{
	uint64_t	v = x & 0xffffu;
	v = ( v | ( v << 24 ) ) & 0x000000ff000000ffull;
	v = ( v | ( v << 12 ) ) & 0x000f000f000f000full;
	v = ( v | ( v << 6 ) ) & 0x0303030303030303ull;
	const uint64_t	b0 = v & 0x0101010101010101ull, b1 = ( v >> 1 ) & 0x0101010101010101ull;
	return 0x6161616161616161ull + 2 * b0 + 6 * b1 + 11 * ( b0 & b1 );
}
// eight bits as eight bytes of 0xff or 0
RMT_FN uint64_t dbtext_bytes8( uint32_t bits )
{
	const uint64_t	y = ( uint64_t( bits & 0xffu ) * 0x0101010101010101ull ) & 0x8040201008040201ull;
	return ( ( ( y + 0x7f7f7f7f7f7f7f7full ) >> 7 ) & 0x0101010101010101ull ) * 0xffull;
}

// The 16 bytes of a slot, out[ 0 ] the first eight: the letters of code word `code`, n where `mask` (the slot's
// masked bases) or `tail` (no bases) has a bit.  Without exceptions that is the slot.
RMT_FN void dbtext_slot_plain( uint32_t code, uint32_t mask, uint32_t tail, uint64_t out[ 2 ] )
{
	const uint32_t	n = mask | tail;
	const uint64_t	m0 = dbtext_bytes8( n ), m1 = dbtext_bytes8( n >> 8 );
	out[ 0 ] = ( dbtext_letters8( code ) & ~m0 ) | ( 0x6e6e6e6e6e6e6e6eull & m0 );
	out[ 1 ] = ( dbtext_letters8( code >> 16 ) & ~m1 ) | ( 0x6e6e6e6e6e6e6e6eull & m1 );
}
// ... and with them: the masked bases of the slot take exc[ idx ], exc[ idx + 1 ], ... in order; an index outside
// [ 0, n_exc ) leaves the n (the per-entry check has refused such a database before its text is trusted)
RMT_FN void dbtext_slot_patch( uint32_t mask, const char *exc, int64_t idx, int64_t n_exc, uint64_t out[ 2 ] )
{
	while( mask != 0 ){
#if defined( __HIP_DEVICE_COMPILE__ )
		const int	j = __ffs( int( mask ) ) - 1;
#else
		const int	j = __builtin_ctz( mask );
#endif
		mask &= mask - 1;
		if( idx >= 0 && idx < n_exc ){
			const int	sh = 8 * ( j & 7 );
			const uint64_t	c = static_cast<unsigned char>( exc[ idx ] );
			out[ j >> 3 ] = ( out[ j >> 3 ] & ~( 0xffull << sh ) ) | ( c << sh );
		}
		idx++;
	}
}

// the slot of the text that byte offset `at` of it lies in belongs to the last entry that starts at or before it
// (entries without bases have no slot): the number of entries among text_start[ lo .. hi ) that start at or before
// `at`, plus lo
RMT_FN int32_t dbtext_entry_at( const int64_t *text_start, int32_t lo, int32_t hi, int64_t at )
{
	while( lo < hi ){
		const int32_t	mid = lo + ( hi - lo ) / 2;
		if( text_start[ mid ] <= at )
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

// the word the check reports through, least first: the entry, then what is wrong with it, then a value --
// DT_BAD_COUNT: the bases its mask has set (its exceptions are another number), DT_BAD_LETTER: the byte
enum { DT_BAD_COUNT = 0, DT_BAD_LETTER = 1 };
RMT_FN unsigned long long dbtext_bad_word( int32_t entry, int kind, uint32_t value )
{
	return ( static_cast<unsigned long long>( static_cast<uint32_t>( entry ) ) << 33 ) | ( static_cast<unsigned long long>( kind ) << 32 ) | value;
}
RMT_FN int32_t dbtext_bad_entry( unsigned long long w ) { return int32_t( w >> 33 ); }
RMT_FN int dbtext_bad_kind( unsigned long long w ) { return int( ( w >> 32 ) & 1 ); }
RMT_FN uint32_t dbtext_bad_value( unsigned long long w ) { return uint32_t( w & 0xffffffffull ); }
constexpr unsigned long long	DT_BAD_NONE = ~0ull;

}	// namespace rma
