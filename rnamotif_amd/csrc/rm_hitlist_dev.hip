// rm_hitlist_dev.hip -- see rm_hitlist_dev.h
#include <algorithm>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "rm_hitlist_dev.h"

namespace rma {

namespace {

constexpr int	HL_BLOCK = 256;
constexpr int	HL_WAVES = HL_BLOCK / 64;
constexpr int	HL_SEG_ROOM = 128;
static_assert( HL_MAX_SEGS <= HL_SEG_ROOM, "two lane passes hold a line's segments" );

// reductions over the 64 lanes of a wave; every lane has the result
__device__ inline unsigned wave_max( unsigned v )
{
	for( int d = 32; d > 0; d >>= 1 )
		v = max( v, unsigned( __shfl_xor( int( v ), d ) ) );
	return v;
}

__device__ inline unsigned wave_min( unsigned v )
{
	for( int d = 32; d > 0; d >>= 1 )
		v = min( v, unsigned( __shfl_xor( int( v ), d ) ) );
	return v;
}

__device__ inline unsigned long long wave_min( unsigned long long v )
{
	for( int d = 32; d > 0; d >>= 1 )
		v = min( v, __shfl_xor( v, d ) );
	return v;
}

__device__ inline unsigned long long wave_sum( unsigned long long v )
{
	for( int d = 32; d > 0; d >>= 1 )
		v += __shfl_xor( v, d );
	return v;
}

// the letters of one record's strand: the entry's text through the call's table (256 letters, 256 complements)
struct ListLet {
	const uint8_t	*entry_p, *letcmp;
	int32_t	comp, slen;
	__device__ uint8_t	letter( int32_t p ) const
	{
		return letcmp[ ( comp ? 256 : 0 ) + entry_p[ hitwin_src( comp, slen, p, 0 ) ] ];
	}
};
typedef HitListView<ListLet>	ListView;

// record h of the call as the rule reads it; r: its measured form
__device__ inline ListView list_view( const HitListCall &c, const uint8_t *text, const uint8_t *letcmp, long long h, const HitListRec *r )
{
	const int32_t	*w = c.hits + h * c.stride;
	const int32_t	entry = w[ 0 ];
	return ListView{ r, w, c.names.bytes + c.names.off[ 2 * int64_t( entry ) ], c.text_bytes + h * ( long long )c.text_width, c.text_len[ h ],
		ListLet{ text + c.start[ entry ], letcmp, w[ 1 ], c.slen[ entry ] } };
}

// One lane per record.  Of a record only its own words are read, of the tables and of its score column only what
// belongs to a record that has passed the check.  Every lane of a wave takes part in the reductions, a lane without a
// printed record with the neutral values.
__global__ void __launch_bounds__( HL_BLOCK )
rma_hit_list_measure_kernel( HitListCall c, long long c0, long long cn, int64_t *flag, HitListSums *sums )
{
	const long long	i = blockIdx.x * ( long long )HL_BLOCK + threadIdx.x;
	const int	lane = threadIdx.x & 63;
	unsigned long long	bad = ~0ull, first = ~0ull, bytes = 0;
	unsigned	k_min = ~0u, k_max = 0, not_number = 0;
	HitListRec	r;
	r.k = -1;
	const int32_t	*w = c.hits;
	if( i < cn ){
		const long long	h = c0 + i;
		w = c.hits + h * c.stride;
		int	which;
		int	code = hitprint_check( w, c.shape, c.n_seq, c.slen, c.text_len[ h ], c.text_width, &which );
		if( code == HW_OK && ( c.accept == nullptr || c.accept[ h ] != 0 ) ){
			const int64_t	*o = c.names.off + 2 * int64_t( w[ 0 ] );
			const HitPrintIn	in{ o[ 1 ] - o[ 0 ], o[ 2 ] - o[ 1 ], c.slen[ w[ 0 ] ], c.text_len[ h ] };
			code = rmlist_measure( w, c.shape, in, c.names.bytes + o[ 0 ], c.text_bytes + h * ( long long )c.text_width, c.name_mode, &r );
			if( code == HW_OK ){
				first = static_cast<unsigned long long>( h );
				bytes = static_cast<unsigned long long>( r.temp_len );
				k_min = k_max = unsigned( r.k );
				not_number = ( r.flags & HL_F_NUMBER ) ? 0u : 1u;
			}else
				r.k = -1;
		}
		if( code != HW_OK )
			bad = static_cast<unsigned long long>( h ) * 16u + unsigned( code );
		c.recs[ h ] = r;
		flag[ i ] = r.k >= 0 ? 1 : 0;
	}else if( i == cn )
		flag[ cn ] = 0;
	const bool	printed = r.k >= 0;
	// (a wave without a printed record and without a refused one has nothing to add)
	bad = wave_min( bad );
	first = wave_min( first );
	if( bad == ~0ull && first == ~0ull )
		return;
	bytes = wave_sum( bytes );
	const unsigned long long	lines = wave_sum( printed ? 1ull : 0ull );
	k_min = wave_min( k_min );
	k_max = wave_max( k_max );
	not_number = wave_max( not_number );
	if( lane == 0 ){
		if( bad != ~0ull )
			atomicMin( &sums->bad, bad );
		if( first != ~0ull ){
			atomicMin( &sums->first, first );
			atomicAdd( &sums->temp_bytes, bytes );
			atomicAdd( &sums->n_lines, lines );
			atomicMin( &sums->k_min, k_min );
			atomicMax( &sums->k_max, k_max );
			if( not_number )
				atomicMax( &sums->not_number, 1u );
		}
	}
	if( first == ~0ull )
		return;
	const int	n_segs = rmlist_n_segs( c.shape );
	for( int g = 0; g < n_segs; g++ ){
		const unsigned	m = wave_max( printed ? unsigned( rmlist_seg_len( r, w, c.shape, g ) ) : 0u );
		if( lane == 0 && m > 0 )
			atomicMax( &sums->width[ g ], m );
	}
}

__global__ void __launch_bounds__( HL_BLOCK )
rma_hit_list_compact_kernel( const int64_t *flag, const int64_t *off, const int64_t *carry, long long c0, long long cn, int64_t *idx )
{
	const long long	i = blockIdx.x * ( long long )HL_BLOCK + threadIdx.x;
	if( i < cn && flag[ i ] != 0 )
		idx[ *carry + off[ i ] ] = c0 + i;
}

__global__ void __launch_bounds__( 256 )
rma_hit_list_letters_kernel( const uint8_t *table, int codes, uint8_t *letcmp )
{
	const int	t = threadIdx.x;
	const unsigned char	v = table[ t ];
	const unsigned char	l = codes ? hitwin_code_letter( v ) : v;
	letcmp[ t ] = l;
	letcmp[ 256 + t ] = hitwin_wc_cmp( l );
}

// rmlist_less over record indices
struct ListLess {
	HitListCall	c;
	const uint8_t	*text, *letcmp;
	int	mode;
	__device__ bool	operator()( const int64_t &a, const int64_t &b ) const
	{
		return rmlist_less( mode, c.shape, list_view( c, text, letcmp, a, c.recs + a ), a, list_view( c, text, letcmp, b, c.recs + b ), b );
	}
};

// A wave per line; the loop over the lines runs the same number of times in every wave of a workgroup, so the
// workgroup's barriers stand between the lanes that lay a line's segment lengths into LDS and the lanes that read
// them.  Nothing outside [ r * line_len, ( r + 1 ) * line_len ) of the output is written for line r, and nothing outside
// its record's entry, name and score column is read: the measure pass has checked the record and counted the same
// segments.
__global__ void __launch_bounds__( HL_BLOCK )
rma_hit_list_fill_kernel( HitListCall c, const uint8_t *text, const uint8_t *letcmp, const HitListLayout *layout, int32_t line_len,
	const int64_t *perm, long long n_lines, uint8_t *out )
{
	__shared__ uint8_t	s_lc[ 512 ];
	__shared__ int32_t	s_off[ HL_SEG_ROOM ], s_width[ HL_SEG_ROOM ];
	__shared__ uint8_t	s_right[ HL_SEG_ROOM ];
	__shared__ int32_t	s_len[ HL_WAVES ][ HL_SEG_ROOM ];
	const int	t = threadIdx.x;
	s_lc[ t ] = letcmp[ t ];
	s_lc[ 256 + t ] = letcmp[ 256 + t ];
	const int	n_segs = rmlist_n_segs( c.shape );
	if( t < HL_SEG_ROOM ){
		const bool	in = t < n_segs;
		s_off[ t ] = in ? layout->off[ t ] : 0;
		s_width[ t ] = in ? layout->width[ t ] : 0;
		s_right[ t ] = in ? layout->right[ t ] : 0;
	}
	const int	lane = t & 63, wave = t >> 6;
	for( long long r0 = blockIdx.x * ( long long )HL_WAVES; r0 < n_lines; r0 += gridDim.x * ( long long )HL_WAVES ){
		const long long	r = r0 + wave;
		const bool	live = r < n_lines;
		const long long	h = live ? perm[ r ] : 0;
		HitListRec	rec;
		if( live ){
			rec = c.recs[ h ];
			const int32_t	*w = c.hits + h * c.stride;
			for( int g = lane; g < n_segs; g += 64 )
				s_len[ wave ][ g ] = rmlist_seg_len( rec, w, c.shape, g );
		}
		__syncthreads();
		if( live ){
			const ListView	v = list_view( c, text, s_lc, h, &rec );
			uint8_t	*dst = out + r * line_len;
			for( int32_t b = lane; b < line_len; b += 64 ){
				uint8_t	x = '\n';
				if( b < line_len - 1 ){
					const int	g = rmlist_find_seg( s_off, n_segs, b );
					x = rmlist_cell_byte( v, c.shape, g, s_len[ wave ][ g ], s_width[ g ], s_right[ g ] != 0, b - s_off[ g ] );
				}
				dst[ b ] = x;
			}
		}
		__syncthreads();
	}
}

}	// namespace

hipError_t hit_list_measure( const HitListCall &c, long long c0, long long cn, int64_t *d_flag, HitListSums *d_sums, hipStream_t s )
{
	if( cn < 0 || c0 < 0 || c0 + cn > c.n )
		return hipErrorInvalidValue;
	hipLaunchKernelGGL( rma_hit_list_measure_kernel, dim3( unsigned( ( cn + 1 + HL_BLOCK - 1 ) / HL_BLOCK ) ), dim3( HL_BLOCK ), 0, s,
		c, c0, cn, d_flag, d_sums );
	return hipGetLastError();
}

hipError_t hit_list_compact( const int64_t *d_flag, const int64_t *d_off, const int64_t *d_carry, long long c0, long long cn, int64_t *d_idx, hipStream_t s )
{
	if( cn <= 0 )
		return cn < 0 ? hipErrorInvalidValue : hipSuccess;
	hipLaunchKernelGGL( rma_hit_list_compact_kernel, dim3( unsigned( ( cn + HL_BLOCK - 1 ) / HL_BLOCK ) ), dim3( HL_BLOCK ), 0, s,
		d_flag, d_off, d_carry, c0, cn, d_idx );
	return hipGetLastError();
}

hipError_t hit_list_letters( const uint8_t *table, int codes, uint8_t *d_letcmp, hipStream_t s )
{
	hipLaunchKernelGGL( rma_hit_list_letters_kernel, dim3( 1 ), dim3( 256 ), 0, s, table, codes, d_letcmp );
	return hipGetLastError();
}

hipError_t hit_list_sort( const HitListCall &c, const uint8_t *text, const uint8_t *d_letcmp, int mode, const int64_t *d_idx, int64_t *d_perm,
	long long n_lines, void *tmp, size_t *tmp_bytes, hipStream_t s )
{
	if( n_lines <= 0 || ( mode != 1 && mode != 2 ) )
		return hipErrorInvalidValue;
	return rocprim::merge_sort( tmp, *tmp_bytes, d_idx, d_perm, size_t( n_lines ), ListLess{ c, text, d_letcmp, mode }, s );
}

hipError_t hit_list_fill( const HitListCall &c, const uint8_t *text, const uint8_t *d_letcmp, const HitListLayout *d_layout, int32_t line_len,
	const int64_t *d_perm, long long n_lines, uint8_t *d_out, hipStream_t s )
{
	if( n_lines <= 0 )
		return n_lines < 0 ? hipErrorInvalidValue : hipSuccess;
	const int64_t	blocks = std::min<int64_t>( ( n_lines + HL_WAVES - 1 ) / HL_WAVES, 2048 );
	hipLaunchKernelGGL( rma_hit_list_fill_kernel, dim3( unsigned( blocks ) ), dim3( HL_BLOCK ), 0, s,
		c, text, d_letcmp, d_layout, line_len, d_perm, n_lines, d_out );
	return hipGetLastError();
}

}	// namespace rma
