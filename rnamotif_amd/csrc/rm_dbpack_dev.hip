// rm_dbpack_dev.hip -- see rm_dbpack_dev.h
//
// One lane per 32-base mask word, a workgroup per PK_WORDS consecutive words (8192 bases):
//  1. one bisection of base_off for the workgroup's first entry and one for the first entry past its
//     words (two lanes of two waves, side by side); the offsets of the entries in between go to LDS
//     and each lane finds its word's entry there (in global memory when more than PK_WORDS entries
//     lie in between: entries of no bases);
//  2. the workgroup's text comes into LDS as dwords, slot j of the stage from lane j % PK_WORDS:
//     consecutive lanes read consecutive, aligned dwords although entries start at any byte (an
//     unaligned dword is two aligned loads and a byte shift; a load is made only where it holds a
//     byte of the entry, so that nothing outside the entry's allocation is read);
//  3. each lane turns its word's 32 bytes into the mask word and two code words through the table
//     (in LDS) and stores them: full words, coalesced.  Bits past the entry's last base are zero.
#include <hip/hip_runtime.h>
#include "rm_dbpack_dev.h"

namespace rma {

namespace {

constexpr int	PK_WORDS = 256;

__global__ void __launch_bounds__( PK_WORDS )
rma_pack_text_kernel( const uint8_t *text, const int64_t *start, const int64_t *base_off, const int32_t *slen, int n,
	long long mask_words, const uint8_t *table, uint32_t *codes, uint32_t *amask )
{
	__shared__ uint32_t	stage[ PK_WORDS * 8 ];	// the workgroup's text, 32 bytes per word
	__shared__ int64_t	bo[ PK_WORDS ];		// base_off of the entries its words lie in
	__shared__ long long	src[ PK_WORDS ];	// per word: its first byte's offset from text
	__shared__ int	nval[ PK_WORDS ];		// per word: bytes of it that are bases (0-32)
	__shared__ uint32_t	tab[ 64 ];
	__shared__ int	ends[ 2 ];
	const int	t = threadIdx.x;
	const long long	w0 = blockIdx.x * ( long long )PK_WORDS, w = w0 + t;
	const long long	w_end = w0 + PK_WORDS < mask_words ? w0 + PK_WORDS : mask_words;
	if( t < 64 )
		tab[ t ] = reinterpret_cast<const uint32_t *>( table )[ t ];
	if( t == 0 ){		// the last entry at or before the first word
		const long long	b = 32 * w0;
		int	lo = 0, hi = n;
		while( lo < hi ){
			const int	mid = ( lo + hi ) >> 1;
			if( base_off[ mid ] <= b )
				lo = mid + 1;
			else
				hi = mid;
		}
		ends[ 0 ] = lo > 0 ? lo - 1 : 0;
	}else if( t == 64 ){	// the first entry that starts past the last word
		const long long	b = 32 * w_end;
		int	lo = 0, hi = n;
		while( lo < hi ){
			const int	mid = ( lo + hi ) >> 1;
			if( base_off[ mid ] < b )
				lo = mid + 1;
			else
				hi = mid;
		}
		ends[ 1 ] = lo;
	}
	__syncthreads();
	const int	e0 = ends[ 0 ], m = ends[ 1 ] - e0;
	if( m <= PK_WORDS && t < m )
		bo[ t ] = base_off[ e0 + t ];
	__syncthreads();
	int	nv = 0;
	if( w < mask_words ){
		const int64_t	*b = m <= PK_WORDS ? bo : base_off + e0;
		int	lo = 0, hi = m;
		while( lo < hi ){
			const int	mid = ( lo + hi ) >> 1;
			if( b[ mid ] <= 32 * w )
				lo = mid + 1;
			else
				hi = mid;
		}
		const int	e = e0 + ( lo > 0 ? lo - 1 : 0 );
		const long long	r = 32 * w - b[ lo > 0 ? lo - 1 : 0 ];
		const long long	left = slen[ e ] - r;
		nv = left < 0 ? 0 : left > 32 ? 32 : int( left );
		src[ t ] = start[ e ] + r;
	}
	nval[ t ] = nv;
	__syncthreads();
	const uintptr_t	base = reinterpret_cast<uintptr_t>( text );
#pragma unroll
	for( int i = 0; i < 8; i++ ){
		const int	j = t + PK_WORDS * i, lw = j >> 3, k = j & 7;
		const int	v = nval[ lw ] - 4 * k;		// bytes of this dword that are bases
		uint32_t	x = 0;
		if( v > 0 ){
			const uintptr_t	a = base + uintptr_t( src[ lw ] ) + uintptr_t( 4 * k );
			const uint32_t	*p = reinterpret_cast<const uint32_t *>( a & ~uintptr_t( 3 ) );
			const unsigned	sh = unsigned( a & 3 );
			const uint32_t	lo = p[ 0 ];
			const uint32_t	hi = int( sh ) + v > 4 ? p[ 1 ] : 0u;
			x = __builtin_amdgcn_alignbyte( hi, lo, sh );
		}
		stage[ j ] = x;
	}
	__syncthreads();
	if( w >= mask_words )
		return;
	const uint4	q0 = *reinterpret_cast<const uint4 *>( &stage[ t * 8 ] );
	const uint4	q1 = *reinterpret_cast<const uint4 *>( &stage[ t * 8 + 4 ] );
	const uint32_t	x[ 8 ] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w };
	const uint8_t	*tb = reinterpret_cast<const uint8_t *>( tab );
	uint32_t	c[ 2 ] = { 0u, 0u }, msk = 0;
#pragma unroll
	for( int k = 0; k < 32; k++ ){
		const unsigned	v = tb[ ( x[ k >> 2 ] >> ( 8 * ( k & 3 ) ) ) & 0xffu ];
		const unsigned	amb = v > 3u ? 1u : 0u;
		c[ k >> 4 ] |= ( amb ? 0u : v ) << ( 2 * ( k & 15 ) );
		msk |= amb << k;
	}
	// (the bytes past the entry's last base are whatever the stage holds: not bases)
	const uint32_t	keep = nv >= 32 ? ~0u : ( 1u << nv ) - 1u;
	const uint32_t	keep0 = nv >= 16 ? ~0u : ( 1u << ( 2 * nv ) ) - 1u;
	const uint32_t	keep1 = nv >= 32 ? ~0u : nv <= 16 ? 0u : ( 1u << ( 2 * ( nv - 16 ) ) ) - 1u;
	reinterpret_cast<uint2 *>( codes )[ w ] = make_uint2( c[ 0 ] & keep0, c[ 1 ] & keep1 );
	amask[ w ] = msk & keep;
}

}	// namespace

hipError_t pack_text( const uint8_t *text, const int64_t *d_start, const int64_t *d_base_off, const int32_t *d_slen, int32_t n,
	int64_t mask_words, const uint8_t *d_table, uint32_t *codes, uint32_t *amask, hipStream_t s )
{
	if( mask_words <= 0 || n <= 0 )
		return hipSuccess;
	hipLaunchKernelGGL( rma_pack_text_kernel, dim3( unsigned( ( mask_words + PK_WORDS - 1 ) / PK_WORDS ) ), dim3( PK_WORDS ), 0, s,
		text, d_start, d_base_off, d_slen, int( n ), ( long long )mask_words, d_table, codes, amask );
	return hipGetLastError();
}

}	// namespace rma
