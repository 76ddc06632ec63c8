// rm_hitalign_dev.hip -- see rm_hitalign_dev.h
#include <algorithm>
#include <hip/hip_runtime.h>
#include "rm_hitalign_dev.h"

namespace rma {

namespace {

constexpr int	HA_BLOCK = 256;
constexpr int	HA_WAVES = HA_BLOCK / 64;
static_assert( HA_MAX_COLS <= 128 && HA_MAX_COLS <= HA_BLOCK, "two lane passes hold a record's columns, one thread copies one column" );

// A wave takes records in turn, grid-stride; lane e keeps the maximum of columns e and 64 + e.  Only length words of
// the records are read, each inside its record.
__global__ void __launch_bounds__( HA_BLOCK )
rma_hit_widths_kernel( const int32_t *hits, long long n, int stride, HitWinShape shape, int32_t *widths )
{
	__shared__ int32_t	wmax[ 128 ];
	const int	t = threadIdx.x, lane = t & 63;
	if( t < 128 )
		wmax[ t ] = 0;
	__syncthreads();
	const int	nc = hitalign_n_cols( shape );
	// the length words of this lane's two columns (-1: no such column)
	const int	ka = lane < nc ? hitstruct_word( shape, hitalign_col_elem( shape, lane ) ) + 1 : -1;
	const int	kb = 64 + lane < nc ? hitstruct_word( shape, hitalign_col_elem( shape, 64 + lane ) ) + 1 : -1;
	int32_t	ma = 0, mb = 0;
	for( long long r = blockIdx.x * ( long long )HA_WAVES + ( t >> 6 ); r < n; r += gridDim.x * ( long long )HA_WAVES ){
		const int32_t	*w = hits + r * stride;
		if( ka >= 0 )
			ma = max( ma, hitalign_width( w[ ka ] ) );
		if( kb >= 0 )
			mb = max( mb, hitalign_width( w[ kb ] ) );
	}
	if( ma > 0 )
		atomicMax( &wmax[ lane ], ma );
	if( mb > 0 )
		atomicMax( &wmax[ 64 + lane ], mb );
	__syncthreads();
	if( t < nc && wmax[ t ] > 0 )
		atomicMax( &widths[ t ], wmax[ t ] );
}

// A wave per record, grid-stride over the records (rm_hitalign_dev.h has the plan).  The loop over a row has the same
// trip count on all lanes of a wave, so the lane shuffles run with the whole wave active; a lane past the row's end
// works on its last byte and stores nothing.  Nothing outside row r of rows / pos is written, and nothing outside the
// record's entry is read: hit_spans has passed, so a letter's position lies inside its element, inside the entry.
__global__ void __launch_bounds__( HA_BLOCK )
rma_hit_align_kernel( const uint8_t *text, const int32_t *hits, long long n, int stride, HitWinShape shape, HitAlignLayout lay,
	const int32_t *slen, const int64_t *start, const uint8_t *table, int codes, uint8_t *rows, int32_t *pos_out )
{
	__shared__ uint8_t	let[ 256 ], cmp[ 256 ];		// byte -> its letter, the complement of its letter
	__shared__ int64_t	c_off[ HA_MAX_COLS ];
	__shared__ int32_t	c_width[ HA_MAX_COLS ];
	__shared__ uint8_t	c_right[ HA_MAX_COLS ];
	const int	t = threadIdx.x;
	{
		const unsigned char	v = table[ t ];
		const unsigned char	l = codes ? hitwin_code_letter( v ) : v;
		let[ t ] = l;
		cmp[ t ] = hitwin_wc_cmp( l );
		if( t < HA_MAX_COLS ){
			c_off[ t ] = lay.off[ t ];
			c_width[ t ] = lay.width[ t ];
			c_right[ t ] = lay.right[ t ];
		}
	}
	__syncthreads();
	const int	lane = t & 63;
	const int	nc = lay.n_cols;
	const int64_t	W = lay.row_bytes;
	const int	nt = shape.n_elems + 2;
	const int	n_a = nt < 64 ? nt : 64, n_b = nt - n_a;	// elements held in the first / second lane pass
	for( long long r = blockIdx.x * ( long long )HA_WAVES + ( t >> 6 ); r < n; r += gridDim.x * ( long long )HA_WAVES ){
		const int32_t	*w = hits + r * stride;
		const int32_t	entry = w[ 0 ], comp = w[ 1 ];
		const int32_t	sl = slen[ entry ];
		const uint8_t	*src = text + start[ entry ];
		// the record's elements, once: lane e has element e and element 64 + e
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
		uint8_t	*row = rows + r * W;
		int32_t	*prow = pos_out != nullptr ? pos_out + r * W : nullptr;
		for( int64_t b0 = 0; b0 < W; b0 += 64 ){
			const int64_t	b = b0 + lane;
			const bool	in = b < W;
			const int64_t	bb = in ? b : W - 1;
			const int	c = hitalign_find_col( c_off, nc, bb );
			const int	e = hitalign_col_elem( shape, c );
			int32_t	e_off = __shfl( off_a, e & 63 ), e_len = __shfl( len_a, e & 63 );
			if( n_b > 0 ){
				const int32_t	o2 = __shfl( off_b, e & 63 ), l2 = __shfl( len_b, e & 63 );
				e_off = e < 64 ? e_off : o2;
				e_len = e < 64 ? e_len : l2;
			}
			int32_t	k;
			const int	kind = hitalign_place( c_width[ c ], c_right[ c ], e_len, bb - c_off[ c ], &k );
			uint8_t	v = hitalign_fill_byte( lay.fill, kind );
			int32_t	p = -1;
			if( kind == HA_LETTER ){
				p = e_off + k;
				const uint8_t	x = src[ hitwin_src( comp, sl, p, 0 ) ];
				v = comp ? cmp[ x ] : let[ x ];
			}
			if( in ){
				row[ b ] = v;
				if( prow != nullptr )
					prow[ b ] = p;
			}
		}
	}
}

}	// namespace

hipError_t hit_align_widths( const int32_t *d_hits, int64_t n, int stride, const HitWinShape &shape, int32_t *d_widths, hipStream_t s )
{
	if( n <= 0 )
		return n < 0 ? hipErrorInvalidValue : hipSuccess;
	const int64_t	blocks = std::min<int64_t>( ( n + HA_WAVES - 1 ) / HA_WAVES, 2048 );
	hipLaunchKernelGGL( rma_hit_widths_kernel, dim3( unsigned( blocks ) ), dim3( HA_BLOCK ), 0, s, d_hits, ( long long )n, stride, shape,
		d_widths );
	return hipGetLastError();
}

hipError_t hit_align_fill( const uint8_t *text, const int32_t *d_hits, int64_t n, int stride, const HitWinShape &shape,
	const HitAlignLayout &lay, const int32_t *d_slen, const int64_t *d_start, const uint8_t *table, int codes, uint8_t *d_rows,
	int32_t *d_pos, hipStream_t s )
{
	if( n <= 0 || lay.row_bytes <= 0 )
		return n < 0 ? hipErrorInvalidValue : hipSuccess;
	// (a few waves per CU: the rows are short, the work is the launch)
	const int64_t	blocks = std::min<int64_t>( ( n + HA_WAVES - 1 ) / HA_WAVES, 2048 );
	hipLaunchKernelGGL( rma_hit_align_kernel, dim3( unsigned( blocks ) ), dim3( HA_BLOCK ), 0, s, text, d_hits, ( long long )n, stride,
		shape, lay, d_slen, d_start, table, codes, d_rows, d_pos );
	return hipGetLastError();
}

}	// namespace rma
