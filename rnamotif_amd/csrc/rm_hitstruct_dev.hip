// rm_hitstruct_dev.hip -- see rm_hitstruct_dev.h
#include <algorithm>
#include <hip/hip_runtime.h>
#include "rm_hitstruct_dev.h"

namespace rma {

namespace {

constexpr int	HS_BLOCK = 256;
constexpr int	HS_WAVES = HS_BLOCK / 64;
constexpr int	HS_TABLE_WORDS = int( sizeof( HitStructTable ) / 4 );
static_assert( sizeof( HitStructTable ) % 4 == 0 && sizeof( HitStructElem ) == 12, "the table is copied word by word" );
static_assert( RMA_MAX_ELEMS + 2 <= 128, "two lane passes hold a record's elements and contexts" );

__global__ void __launch_bounds__( HS_BLOCK )
rma_hit_helix_kernel( const int32_t *hits, long long n, int stride, const HitStructTable *tab, unsigned long long *bad )
{
	const long long	h = blockIdx.x * ( long long )HS_BLOCK + threadIdx.x;
	if( h >= n )
		return;
	const int32_t	*w = hits + h * stride;
	const int	ne = tab->n_elems;
	for( int e = 0; e < ne; e++ ){
		const HitStructElem	x = tab->e[ e ];
		if( x.n_strands < 2 || x.self == 0 )
			continue;
		if( w[ RMA_HIT_HDR + 4 * e + 1 ] != w[ RMA_HIT_HDR + 4 * x.strand[ 0 ] + 1 ] ){
			atomicMin( bad, static_cast<unsigned long long>( h ) );
			return;
		}
	}
}

__global__ void rma_hit_carry_kernel( int64_t *carry, const int64_t *add )
{
	if( blockIdx.x == 0 && threadIdx.x == 0 )
		*carry += *add;
}

// A wave per record, grid-stride over the records (rm_hitstruct_dev.h has the plan).  Every loop below has the same
// trip count on all lanes of a wave, so the lane reads and shuffles run with the whole wave active.  Nothing outside
// the record's window is written and nothing outside its entry is read: hit_spans and the helix check have passed.
__global__ void __launch_bounds__( HS_BLOCK )
rma_hit_struct_kernel( const uint8_t *text, const int32_t *hits, long long n, int stride, HitWinShape shape, const HitStructTable *g_tab,
	const int32_t *lo_in, const int64_t *src_in, const int64_t *offc, const int64_t *carry, const uint8_t *table, int codes,
	HitStructOut out, int last )
{
	__shared__ uint8_t	let[ 256 ], cmp[ 256 ];		// byte -> its letter, the complement of its letter
	__shared__ HitStructTable	tab;
	const int	t = threadIdx.x;
	{
		const unsigned char	v = table[ t ];
		const unsigned char	l = codes ? hitwin_code_letter( v ) : v;
		let[ t ] = l;
		cmp[ t ] = hitwin_wc_cmp( l );
		const int32_t	*g = reinterpret_cast<const int32_t *>( g_tab );
		int32_t	*s = reinterpret_cast<int32_t *>( &tab );
		for( int k = t; k < HS_TABLE_WORDS; k += HS_BLOCK )
			s[ k ] = g[ k ];
	}
	__syncthreads();
	const int	lane = t & 63;
	const int	ne = shape.n_elems, nt = ne + 2;
	const int	n_a = nt < 64 ? nt : 64, n_b = nt - n_a;	// elements held in the first / second lane pass
	const int64_t	before = *carry;
	for( long long r = blockIdx.x * ( long long )HS_WAVES + ( t >> 6 ); r < n; r += gridDim.x * ( long long )HS_WAVES ){
		const int64_t	oc = offc[ r ], m = offc[ r + 1 ] - oc, o = before + oc;
		const int32_t	lo = lo_in[ r ];
		if( lane == 0 ){
			out.off[ r ] = o;
			out.lo[ r ] = lo;
			if( last && r == n - 1 )
				out.off[ n ] = o + m;
		}
		if( m <= 0 )
			continue;
		// the record's elements, once: lane e has element e and element 64 + e (length 0: not there)
		const int32_t	*w = hits + r * stride;
		int32_t	off_a = 0, len_a = 0, off_b = 0, len_b = 0;
		if( lane < n_a && hitstruct_present( shape, lane ) ){
			const int	k = hitstruct_word( shape, lane );
			off_a = w[ k ];
			len_a = w[ k + 1 ];
		}
		if( lane < n_b && hitstruct_present( shape, 64 + lane ) ){
			const int	k = hitstruct_word( shape, 64 + lane );
			off_b = w[ k ];
			len_b = w[ k + 1 ];
		}
		const int64_t	src = src_in[ r ];
		for( int64_t i0 = 0; i0 < m; i0 += 64 ){
			const int64_t	i = i0 + lane;
			const bool	in = i < m;
			const int32_t	p = in ? int32_t( lo + i ) : lo;
			// elem: downwards, so that the lowest index that covers p stays
			int	e = -1;
			int32_t	e_off = 0, e_len = 0;
			for( int c = n_b - 1; c >= 0; c-- ){
				const int32_t	co = __builtin_amdgcn_readlane( off_b, c ), cl = __builtin_amdgcn_readlane( len_b, c );
				if( hitstruct_covers( co, cl, p ) ){
					e = 64 + c;
					e_off = co;
					e_len = cl;
				}
			}
			for( int c = n_a - 1; c >= 0; c-- ){
				const int32_t	co = __builtin_amdgcn_readlane( off_a, c ), cl = __builtin_amdgcn_readlane( len_a, c );
				if( hitstruct_covers( co, cl, p ) ){
					e = c;
					e_off = co;
					e_len = cl;
				}
			}
			// mates: the helix from the table, its strands' offsets from the lanes that hold them
			const bool	helix = in && e >= 0 && e < ne && tab.e[ e ].n_strands >= 2;
			const HitStructElem	x = tab.e[ helix ? e : 0 ];
			int32_t	soff[ 4 ];
			for( int q = 0; q < 4; q++ ){
				const int	d = helix && q < x.n_strands ? x.strand[ q ] : 0;
				const int32_t	a = __shfl( off_a, d & 63 );
				int32_t	b = 0;
				if( n_b > 0 )
					b = __shfl( off_b, d & 63 );
				soff[ q ] = d < 64 ? a : b;
			}
			int32_t	mate[ 3 ] = { -1, -1, -1 };
			if( helix )
				hitstruct_mates( x, p - e_off, e_len, soff, lo, mate );
			if( in ){
				const int64_t	at = src >= 0 ? src + i : -1 - src - i;
				const uint8_t	b = text[ at ];
				out.base[ o + i ] = src >= 0 ? let[ b ] : cmp[ b ];
				out.elem[ o + i ] = int16_t( e );
			}
			// mate[ 64 ][ 3 ] of this pass out in three runs of 64 consecutive words
			int32_t	*dst = out.mate + 3 * ( o + i0 );
			const int64_t	words = 3 * ( m - i0 );
			for( int j = 0; j < 3; j++ ){
				const int	wd = j * 64 + lane, from = wd / 3, c = wd - 3 * from;
				const int32_t	v0 = __shfl( mate[ 0 ], from ), v1 = __shfl( mate[ 1 ], from ), v2 = __shfl( mate[ 2 ], from );
				if( wd < words )
					dst[ wd ] = c == 0 ? v0 : c == 1 ? v1 : v2;
			}
		}
	}
}

}	// namespace

hipError_t hit_helix_check( const int32_t *d_hits, int64_t n, int stride, const HitStructTable *d_table, unsigned long long *d_bad,
	hipStream_t s )
{
	if( n <= 0 )
		return n < 0 ? hipErrorInvalidValue : hipSuccess;
	hipLaunchKernelGGL( rma_hit_helix_kernel, dim3( unsigned( ( n + HS_BLOCK - 1 ) / HS_BLOCK ) ), dim3( HS_BLOCK ), 0, s,
		d_hits, ( long long )n, stride, d_table, d_bad );
	return hipGetLastError();
}

hipError_t hit_carry_add( int64_t *d_carry, const int64_t *d_add, hipStream_t s )
{
	hipLaunchKernelGGL( rma_hit_carry_kernel, dim3( 1 ), dim3( 64 ), 0, s, d_carry, d_add );
	return hipGetLastError();
}

hipError_t hit_struct_fill( const uint8_t *text, const int32_t *d_hits, int64_t n, int stride, const HitWinShape &shape,
	const HitStructTable *d_table, const int32_t *d_lo, const int64_t *d_src, const int64_t *d_offc, const int64_t *d_carry,
	const uint8_t *table, int codes, const HitStructOut &out, bool last, hipStream_t s )
{
	if( n <= 0 )
		return hipSuccess;
	// (a few waves per CU: the windows are short, the work is the launch)
	const int64_t	blocks = std::min<int64_t>( ( n + HS_WAVES - 1 ) / HS_WAVES, 2048 );
	hipLaunchKernelGGL( rma_hit_struct_kernel, dim3( unsigned( blocks ) ), dim3( HS_BLOCK ), 0, s,
		text, d_hits, ( long long )n, stride, shape, d_table, d_lo, d_src, d_offc, d_carry, table, codes, out, last ? 1 : 0 );
	return hipGetLastError();
}

}	// namespace rma
