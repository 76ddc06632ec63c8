// rm_hitwin_dev.hip -- see rm_hitwin_dev.h
#include <algorithm>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "rm_hitwin_dev.h"

namespace rma {

namespace {

constexpr int	HW_BLOCK = 256;
constexpr int	HW_WAVES = HW_BLOCK / 64;

__global__ void __launch_bounds__( HW_BLOCK )
rma_hit_span_kernel( const int32_t *hits, long long n, int stride, HitWinShape shape, const int32_t *slen, const int64_t *start,
	int n_seq, int32_t *lo_out, int64_t *len_out, int64_t *src_out, unsigned long long *bad )
{
	const long long	h = blockIdx.x * ( long long )HW_BLOCK + threadIdx.x;
	if( h > n )
		return;
	if( h == n ){
		if( len_out != nullptr )
			len_out[ n ] = 0;
		return;
	}
	int32_t	lo, hi;
	int	which;
	const int	r = hitwin_span( hits + h * stride, shape, n_seq, slen, &lo, &hi, &which );
	if( r != HW_OK )
		atomicMin( bad, static_cast<unsigned long long>( h ) );
	if( len_out != nullptr ){
		const int64_t	m = r == HW_OK ? hitwin_len( lo, hi ) : 0;
		len_out[ h ] = m;
		lo_out[ h ] = lo;
		// the window's first byte in the text, strand 1 as -1 - (that byte), read downwards: the gather kernel
		// reads nothing of the record itself
		int64_t	src = 0;
		if( m > 0 ){
			const int	e = hits[ h * stride ], comp = hits[ h * stride + 1 ];
			src = start[ e ] + hitwin_src( comp, slen[ e ], lo, 0 );
			src = comp ? -1 - src : src;
		}
		src_out[ h ] = src;
	}
}

// A wave per record, grid-stride over the records; the lanes take consecutive bytes of the window, so the
// reads of a wave are one contiguous run of the text (descending on strand 1) and its stores one run of the
// output.  Nothing outside [start, start + slen) of the record's entry is read: its span lies inside the entry
// (hit_spans checked it and wrote where the window starts).
__global__ void __launch_bounds__( HW_BLOCK )
rma_hit_gather_kernel( const uint8_t *text, long long n, const int64_t *src_in, const int64_t *off, const uint8_t *table, int codes,
	uint8_t *out )
{
	__shared__ uint8_t	let[ 256 ], cmp[ 256 ];		// byte -> its letter, the complement of its letter
	const int	t = threadIdx.x;
	{
		const unsigned char	v = table[ t ];
		const unsigned char	l = codes ? hitwin_code_letter( v ) : v;
		let[ t ] = l;
		cmp[ t ] = hitwin_wc_cmp( l );
	}
	__syncthreads();
	const int	lane = t & 63;
	const long long	base = off[ 0 ];
	for( long long r = blockIdx.x * ( long long )HW_WAVES + ( t >> 6 ); r < n; r += gridDim.x * ( long long )HW_WAVES ){
		const int64_t	o = off[ r ], m = off[ r + 1 ] - o;
		if( m <= 0 )
			continue;
		const int64_t	p = src_in[ r ];
		uint8_t	*dst = out + ( o - base );
		if( p >= 0 ){
			const uint8_t	*src = text + p;
			for( int64_t i = lane; i < m; i += 64 )
				dst[ i ] = let[ src[ i ] ];
		}else{
			const uint8_t	*src = text + ( -1 - p );
			for( int64_t i = lane; i < m; i += 64 )
				dst[ i ] = cmp[ *( src - i ) ];
		}
	}
}

}	// namespace

hipError_t hit_spans( const int32_t *d_hits, int64_t n, int stride, const HitWinShape &shape, const int32_t *d_slen,
	const int64_t *d_start, int32_t n_seq, int32_t *d_lo, int64_t *d_len, int64_t *d_src, unsigned long long *d_bad, hipStream_t s )
{
	if( n < 0 )
		return hipErrorInvalidValue;
	hipLaunchKernelGGL( rma_hit_span_kernel, dim3( unsigned( ( n + 1 + HW_BLOCK - 1 ) / HW_BLOCK ) ), dim3( HW_BLOCK ), 0, s,
		d_hits, ( long long )n, stride, shape, d_slen, d_start, int( n_seq ), d_lo, d_len, d_src, d_bad );
	return hipGetLastError();
}

hipError_t hit_offsets( const int64_t *d_len, int64_t *d_off, int64_t n_plus_1, void *tmp, size_t *tmp_bytes, hipStream_t s )
{
	return rocprim::exclusive_scan( tmp, *tmp_bytes, d_len, d_off, int64_t( 0 ), size_t( n_plus_1 ), rocprim::plus<int64_t>(), s );
}

hipError_t hit_gather( const uint8_t *text, int64_t n, const int64_t *d_src, const int64_t *d_off, const uint8_t *table, int codes,
	uint8_t *d_out, hipStream_t s )
{
	if( n <= 0 )
		return hipSuccess;
	// (a few waves per CU: the windows are short, the work is the launch)
	const int64_t	blocks = std::min<int64_t>( ( n + HW_WAVES - 1 ) / HW_WAVES, 2048 );
	hipLaunchKernelGGL( rma_hit_gather_kernel, dim3( unsigned( blocks ) ), dim3( HW_BLOCK ), 0, s,
		text, ( long long )n, d_src, d_off, table, codes, d_out );
	return hipGetLastError();
}

}	// namespace rma
