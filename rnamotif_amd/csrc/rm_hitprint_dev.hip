// rm_hitprint_dev.hip -- see rm_hitprint_dev.h
#include <algorithm>
#include <hip/hip_runtime.h>
#include "rm_hitprint_dev.h"

namespace rma {

namespace {

constexpr int	HP_BLOCK = 256;
constexpr int	HP_WAVES = HP_BLOCK / 64;
constexpr int	HP_SEG_ROOM = 128;
static_assert( HP_MAX_SEGS <= HP_SEG_ROOM, "two lane passes hold a record's segments" );

__device__ inline HitPrintIn print_in( const HitPrintBatch &b, long long h, int32_t entry )
{
	const int64_t	*o = b.names.off + 2 * int64_t( entry );
	return HitPrintIn{ o[ 1 ] - o[ 0 ], o[ 2 ] - o[ 1 ], b.slen[ entry ], b.text_len[ h ] };
}

// One lane per record.  Of a record only its own words are read, of the tables only the slots of an entry that has
// passed the check.
__global__ void __launch_bounds__( HP_BLOCK )
rma_hit_print_size_kernel( HitPrintBatch b, int64_t *len_out, unsigned long long *bad, unsigned long long *bad_text )
{
	const long long	h = blockIdx.x * ( long long )HP_BLOCK + threadIdx.x;
	if( h > b.n )
		return;
	if( h == b.n ){
		len_out[ b.n ] = 0;
		return;
	}
	const int32_t	*w = b.hits + h * b.stride;
	int	which;
	const int	r = hitprint_check( w, b.shape, b.n_seq, b.slen, b.text_len[ h ], b.text_width, &which );
	int64_t	m = 0;
	if( r == HP_TEXT )
		atomicMin( bad_text, static_cast<unsigned long long>( b.first + h ) );
	else if( r != HW_OK )
		atomicMin( bad, static_cast<unsigned long long>( b.first + h ) );
	else
		m = hitprint_size( w, b.shape, print_in( b, h, w[ 0 ] ), b.accept == nullptr || b.accept[ h ] != 0 );
	len_out[ h ] = m;
}

// what hitprint_seg_byte reads, for one record
struct PrintSrc {
	const uint8_t	*sid_p, *sdef_p, *score_p, *num_p, *entry_p, *let, *cmp;
	int32_t	comp, slen;
	__device__ uint8_t	sid( int64_t j ) const { return sid_p[ j ]; }
	__device__ uint8_t	sdef( int64_t j ) const { return sdef_p[ j ]; }
	__device__ uint8_t	score( int64_t j ) const { return score_p[ j ]; }
	__device__ uint8_t	num( int64_t j ) const { return num_p[ j ]; }
	__device__ uint8_t	letter( int32_t p ) const
	{
		const uint8_t	x = entry_p[ hitwin_src( comp, slen, p, 0 ) ];
		return comp ? cmp[ x ] : let[ x ];
	}
};

// A wave per record; the loop over the records runs the same number of times in every wave of a workgroup, so the
// workgroup's barriers stand between the lanes that lay a record's segments into LDS and the lanes that read them.  A
// record of no bytes (not accepted) has only its offset written.  Nothing outside [ *carry + offc[ r ], *carry +
// offc[ r + 1 ] ) of the output is written for record r, and nothing outside its entry, its names and its score column
// is read: the size kernel has checked the record and its text_len, and has counted the same segments.
__global__ void __launch_bounds__( HP_BLOCK )
rma_hit_print_kernel( HitPrintBatch b, const uint8_t *text, const uint8_t *table, int codes, const uint8_t *text_bytes,
	const int64_t *offc, const int64_t *carry, uint8_t *out, int64_t *off_out, int last )
{
	__shared__ uint8_t	let[ 256 ], cmp[ 256 ];		// byte -> its letter, the complement of its letter
	__shared__ int64_t	s_off[ HP_WAVES ][ HP_SEG_ROOM ];	// a segment's first byte
	__shared__ int32_t	s_kind[ HP_WAVES ][ HP_SEG_ROOM ], s_arg[ HP_WAVES ][ HP_SEG_ROOM ];
	__shared__ uint8_t	s_num[ HP_WAVES ][ HP_NUM_CAP ];
	const int	t = threadIdx.x;
	{
		const unsigned char	v = table[ t ];
		const unsigned char	l = codes ? hitwin_code_letter( v ) : v;
		let[ t ] = l;
		cmp[ t ] = hitwin_wc_cmp( l );
	}
	const int	lane = t & 63, wave = t >> 6;
	const int	nseg = hitprint_n_segs( b.shape );
	const int64_t	before = *carry;
	for( long long r0 = blockIdx.x * ( long long )HP_WAVES; r0 < b.n; r0 += gridDim.x * ( long long )HP_WAVES ){
		const long long	r = r0 + wave;
		int64_t	o = 0, m = 0;
		if( r < b.n ){
			o = offc[ r ];
			m = offc[ r + 1 ] - o;
			if( lane == 0 ){
				off_out[ r ] = before + o;
				if( last && r == b.n - 1 )
					off_out[ b.n ] = before + offc[ b.n ];
			}
		}
		const bool	live = m > 0;
		const int32_t	*w = b.hits + ( live ? r : 0 ) * b.stride;
		HitPrintIn	in{ 0, 0, 0, 0 };
		int32_t	entry = 0;
		if( live ){
			entry = w[ 0 ];
			in = print_in( b, r, entry );
			// the digits, once
			int	num_len = 0;
			if( lane == 0 )
				num_len = hitprint_numbers( w, b.shape, in.slen, s_num[ wave ], HP_NUM_CAP );
			num_len = __shfl( num_len, 0 );
			// the segments: lane k has segment k and segment 64 + k; an inclusive prefix over each pass
			HitPrintSeg	ga{ HP_CONST, 0, 0 }, gb{ HP_CONST, 0, 0 };
			if( lane < nseg )
				ga = hitprint_seg( w, b.shape, in, num_len, lane );
			if( 64 + lane < nseg )
				gb = hitprint_seg( w, b.shape, in, num_len, 64 + lane );
			long long	xa = ga.len, xb = gb.len;
			for( int d = 1; d < 64; d <<= 1 ){
				const long long	ua = __shfl_up( xa, d ), ub = __shfl_up( xb, d );
				if( lane >= d ){
					xa += ua;
					xb += ub;
				}
			}
			xb += __shfl( xa, 63 );
			s_off[ wave ][ lane ] = xa - ga.len;
			s_kind[ wave ][ lane ] = ga.kind;
			s_arg[ wave ][ lane ] = ga.arg;
			s_off[ wave ][ 64 + lane ] = xb - gb.len;
			s_kind[ wave ][ 64 + lane ] = gb.kind;
			s_arg[ wave ][ 64 + lane ] = gb.arg;
		}
		__syncthreads();
		if( live ){
			const int64_t	*no = b.names.off + 2 * int64_t( entry );
			// (text_bytes are the call's rows, not the chunk's: record r of the chunk is the call's record first + r)
			const PrintSrc	src{ b.names.bytes + no[ 0 ], b.names.bytes + no[ 1 ], text_bytes + ( b.first + r ) * ( long long )b.text_width, s_num[ wave ],
				text + b.start[ entry ], let, cmp, w[ 1 ], in.slen };
			uint8_t	*dst = out + before + o;
			for( int64_t i = lane; i < m; i += 64 ){
				const int	k = hitprint_find_seg( s_off[ wave ], nseg, i );
				const HitPrintSeg	g{ s_kind[ wave ][ k ], s_arg[ wave ][ k ], 0 };
				dst[ i ] = hitprint_seg_byte( w, g, i - s_off[ wave ][ k ], src );
			}
		}
		__syncthreads();
	}
}

}	// namespace

hipError_t hit_print_sizes( const HitPrintBatch &b, int64_t *d_len, unsigned long long *d_bad, unsigned long long *d_bad_text, hipStream_t s )
{
	if( b.n < 0 )
		return hipErrorInvalidValue;
	hipLaunchKernelGGL( rma_hit_print_size_kernel, dim3( unsigned( ( b.n + 1 + HP_BLOCK - 1 ) / HP_BLOCK ) ), dim3( HP_BLOCK ), 0, s,
		b, d_len, d_bad, d_bad_text );
	return hipGetLastError();
}

hipError_t hit_print_fill( const HitPrintBatch &b, const uint8_t *text, const uint8_t *table, int codes, const uint8_t *text_bytes,
	const int64_t *d_offc, const int64_t *d_carry, uint8_t *d_out, int64_t *d_off, bool last, hipStream_t s )
{
	if( b.n <= 0 )
		return b.n < 0 ? hipErrorInvalidValue : hipSuccess;
	// (a few waves per CU: the lines are short, the work is the launch)
	const int64_t	blocks = std::min<int64_t>( ( b.n + HP_WAVES - 1 ) / HP_WAVES, 2048 );
	hipLaunchKernelGGL( rma_hit_print_kernel, dim3( unsigned( blocks ) ), dim3( HP_BLOCK ), 0, s,
		b, text, table, codes, text_bytes, d_offc, d_carry, d_out, d_off, last ? 1 : 0 );
	return hipGetLastError();
}

}	// namespace rma
