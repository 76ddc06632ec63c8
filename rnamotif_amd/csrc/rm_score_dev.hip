// rm_score_dev.hip -- see rm_score_dev.h.  Compiled with -ffp-contract=off: a double comes out bit for bit as on the host.
#include <hip/hip_runtime.h>
#define RMS_POD_ONLY
#define RMD_FN		static __device__ inline
#define RMD_FN_MEMBER	__device__ inline
#include "rm_score_core.h"
#include "rm_score_dev.h"

namespace rma {

namespace {

constexpr int	SC_MAX_WAVES = 4;

template< bool TEXT, bool MATCH = false > __device__ inline void score_body( const ScoreBatch &b )
{
	extern __shared__ __attribute__(( aligned( 16 ) )) uint64_t	lds[];
	const int	t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int	image_words = b.image_bytes / 8;
	for( int i = t; i < image_words; i += blockDim.x )
		lds[ i ] = static_cast<const uint64_t *>( b.image )[ i ];
	uint8_t	*let = reinterpret_cast<uint8_t *>( lds + image_words ), *cmp = let + 256;
	for( int i = t; i < 256; i += blockDim.x ){
		const unsigned char	v = b.table[ i ];
		const unsigned char	l = b.codes ? hitwin_code_letter( v ) : v;
		let[ i ] = l;
		cmp[ i ] = hitwin_wc_cmp( l );
	}
	__syncthreads();
	const RmsImage	*m = reinterpret_cast<const RmsImage *>( lds );
	const long long	h = blockIdx.x * ( long long )blockDim.x + t;
	if( h >= b.n )
		return;
	const int32_t	*w = b.hits + h * b.stride;
	RmsResult	r;
	r.outcome = RMS_REJECT;
	r.kind = RMS_KIND_NONE;
	r.score = 0.0;
	int32_t	lo, hi;
	int	which;
	if( hitwin_span( w, b.shape, b.n_seq, b.slen, &lo, &hi, &which ) != HW_OK )
		atomicMin( b.bad, static_cast<unsigned long long>( b.first + h ) );
	else{
		const int	wave_words = ( MATCH ? rms_wave_bytes( b.stack, b.n_vars, b.frames ) : rms_wave_bytes( b.stack, b.n_vars ) ) / 4;
		int32_t	*planes = reinterpret_cast<int32_t *>( cmp + 256 ) + wave * wave_words;
		RmsMem<64>	mem{ planes + lane, reinterpret_cast<uint8_t *>( planes + ( b.stack + b.n_vars ) * 3 * 64 ) + lane, b.stack, b.n_vars };
		if( MATCH ){
			// the matcher's planes behind the wave's own: slot k of lane l at word k * 64 + l
			mem.mq = planes + rms_wave_bytes( b.stack, b.n_vars ) / 4 + lane;
			mem.mq_frames = b.frames;
		}
		const int	seq = w[ 0 ], slen = b.slen[ seq ];
		const ScoreBases	bases{ b.text + b.start[ seq ], let, cmp, w[ 1 ], slen };
		if( TEXT ){
			RmsText	tx;
			tx.bits_tab = b.bits_tab;
			if( b.col != nullptr ){
				tx.row = b.col + h * b.col_stride;
				tx.row_cap = b.col_stride;
			}
			if( b.heap != nullptr ){
				const long long	heap_words = ( b.heap_cap + 3 ) / 4;
				mem.heap = b.heap + ( ( h >> 6 ) * 64 * heap_words + lane ) * 4;
				mem.heap_cap = b.heap_cap;
			}
			if( MATCH )
				rms_run_t<true, true>( m, w, slen, bases, mem, b.budget, &r, tx );
			else
				rms_run( m, w, slen, bases, mem, b.budget, &r, tx );
		}else if( MATCH )
			rms_run_t<false, true>( m, w, slen, bases, mem, b.budget, &r, RmsText() );
		else
			rms_run( m, w, slen, bases, mem, b.budget, &r );
		if( r.outcome == RMS_STOPPED ){
			atomicMin( b.stopped, static_cast<unsigned long long>( b.first + h ) );
			if( b.detail != nullptr )
				*b.detail = r;
		}
	}
	const bool	ok = r.outcome == RMS_ACCEPT;
	b.accept[ h ] = ok ? 1 : 0;
	b.score[ h ] = ok ? r.score : 0.0;
	b.kind[ h ] = ok ? int8_t( r.kind ) : int8_t( 0 );
	if( TEXT && b.col_len != nullptr )
		b.col_len[ h ] = ok ? r.text_len : 0;
}

__global__ void __launch_bounds__( SC_MAX_WAVES * 64 )
rma_score_kernel( ScoreBatch b )
{
	score_body<false>( b );
}

__global__ void __launch_bounds__( SC_MAX_WAVES * 64 )
rma_score_text_kernel( ScoreBatch b )
{
	score_body<true>( b );
}

// the two for an image with expressions (RMS_IMG_MATCH and a =~, a !~ or a mismatches( string, pattern ) in MAIN)
__global__ void __launch_bounds__( SC_MAX_WAVES * 64 )
rma_score_match_kernel( ScoreBatch b )
{
	score_body<false, true>( b );
}

__global__ void __launch_bounds__( SC_MAX_WAVES * 64 )
rma_score_match_text_kernel( ScoreBatch b )
{
	score_body<true, true>( b );
}

__global__ void __launch_bounds__( 256 )
rma_score_text_copy_kernel( uint8_t *dst, const uint8_t *src, const int32_t *len, long long n, int stride )
{
	const long long	i = blockIdx.x * ( long long )blockDim.x + threadIdx.x;
	if( i >= n * stride )
		return;
	const long long	h = i / stride;
	if( int( i - h * stride ) < len[ h ] )
		dst[ i ] = src[ i ];
}

}	// namespace

int score_waves( int image_bytes, int stack, int n_vars, int frames )
{
	const int	room = RMS_LDS_BYTES - RMS_LDS_TABLES - image_bytes, wave = rms_wave_bytes( stack, n_vars, frames );
	const int	n = room < wave ? 0 : room / wave;
	return n > SC_MAX_WAVES ? SC_MAX_WAVES : n;
}

hipError_t score_records( const ScoreBatch &b, hipStream_t s )
{
	if( b.n <= 0 )
		return hipSuccess;
	const int	frames = b.match_kernel ? b.frames : -1;
	const int	waves = score_waves( b.image_bytes, b.stack, b.n_vars, frames );
	if( waves < 1 || b.image_bytes % 8 != 0 || b.stack < 1 || b.n_vars < 1 || ( b.match_kernel && ( b.frames < 0 || b.frames > RMQ_MAX_OPS ) ) )
		return hipErrorInvalidValue;
	const int	block = waves * 64;
	const size_t	lds = size_t( b.image_bytes ) + RMS_LDS_TABLES + size_t( waves ) * size_t( rms_wave_bytes( b.stack, b.n_vars, frames ) );
	if( lds > size_t( RMS_LDS_BYTES ) )
		return hipErrorInvalidValue;
	if( b.text_kernel ){
		if( b.heap_cap < 0 || ( b.heap_cap > 0 && b.heap == nullptr ) || ( b.col != nullptr && ( b.col_stride < 1 || b.col_len == nullptr ) ) )
			return hipErrorInvalidValue;
		if( b.match_kernel )
			hipLaunchKernelGGL( rma_score_match_text_kernel, dim3( unsigned( ( b.n + block - 1 ) / block ) ), dim3( unsigned( block ) ), lds, s, b );
		else
			hipLaunchKernelGGL( rma_score_text_kernel, dim3( unsigned( ( b.n + block - 1 ) / block ) ), dim3( unsigned( block ) ), lds, s, b );
	}else if( b.match_kernel )
		hipLaunchKernelGGL( rma_score_match_kernel, dim3( unsigned( ( b.n + block - 1 ) / block ) ), dim3( unsigned( block ) ), lds, s, b );
	else
		hipLaunchKernelGGL( rma_score_kernel, dim3( unsigned( ( b.n + block - 1 ) / block ) ), dim3( unsigned( block ) ), lds, s, b );
	return hipGetLastError();
}

size_t score_heap_bytes( long long n, int heap_cap )
{
	return size_t( ( n + 63 ) / 64 ) * 64 * size_t( ( heap_cap + 3 ) / 4 ) * 4;
}

hipError_t score_text_copy( uint8_t *dst, const uint8_t *src, const int32_t *len, long long n, int stride, hipStream_t s )
{
	if( n <= 0 || stride <= 0 )
		return hipSuccess;
	const long long	total = n * stride;
	hipLaunchKernelGGL( rma_score_text_copy_kernel, dim3( unsigned( ( total + 255 ) / 256 ) ), dim3( 256 ), 0, s, dst, src, len, n, stride );
	return hipGetLastError();
}

hipError_t score_kernel_attributes( int *private_bytes, int *static_lds, int *regs, bool text, bool match )
{
	hipFuncAttributes	a;
	const void	*k = match ? ( text ? reinterpret_cast<const void *>( rma_score_match_text_kernel ) : reinterpret_cast<const void *>( rma_score_match_kernel ) ) :
		( text ? reinterpret_cast<const void *>( rma_score_text_kernel ) : reinterpret_cast<const void *>( rma_score_kernel ) );
	const hipError_t	e = hipFuncGetAttributes( &a, k );
	if( e == hipSuccess ){
		*private_bytes = int( a.localSizeBytes );
		*static_lds = int( a.sharedSizeBytes );
		*regs = a.numRegs;
	}
	return e;
}

}	// namespace rma
