// rm_seqcheck_dev.hip -- see rm_seqcheck_dev.h.
#include <hip/hip_runtime.h>
#define RMQ_POD_ONLY
#define RMS_POD_ONLY
#include "rm_seqcheck.h"
#include "rm_seqcheck_dev.h"
#include "rm_score_dev.h"

namespace rma {

namespace {

__global__ void __launch_bounds__( RMQ_MAX_WAVES * 64 )
rma_seqcheck_kernel( SeqBatch b )
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
	// the workgroup's rows as they are: the rule then writes the words it fixes
	const long long	h0 = blockIdx.x * ( long long )blockDim.x;
	if( b.fixed != nullptr ){
		const long long	rows = b.n - h0 < ( long long )blockDim.x ? b.n - h0 : ( long long )blockDim.x;
		const long long	words = rows * b.stride, at = h0 * b.stride;
		for( long long i = t; i < words; i += blockDim.x )
			b.fixed[ at + i ] = b.hits[ at + i ];
	}
	__syncthreads();
	const RmqImage	*m = reinterpret_cast<const RmqImage *>( lds );
	const long long	h = h0 + t;
	if( h >= b.n )
		return;
	const int32_t	*w = b.hits + h * b.stride;
	RmqResult	r;
	r.outcome = RMQ_DROP;
	r.elem = -1;
	r.steps = 0;
	int32_t	lo, hi;
	int	which;
	if( hitwin_span( w, b.shape, b.n_seq, b.slen, &lo, &hi, &which ) != HW_OK )
		atomicMin( b.bad, static_cast<unsigned long long>( b.first + h ) );
	else{
		const int	wave_words = rmq_wave_bytes( b.frames ) / 4;
		int32_t	*planes = reinterpret_cast<int32_t *>( cmp + 256 ) + wave * wave_words;
		const RmqMem<64>	mem{ planes + lane, b.frames };
		const int	seq = w[ 0 ], slen = b.slen[ seq ];
		const ScoreBases	bases{ b.text + b.start[ seq ], let, cmp, w[ 1 ], slen };
		rmq_run( m, w, bases, mem, b.budget, b.fixed != nullptr ? b.fixed + h * b.stride : nullptr, &r );
		if( r.outcome == RMQ_STOPPED ){
			atomicMin( b.stopped, static_cast<unsigned long long>( b.first + h ) );
			if( b.detail != nullptr )
				*b.detail = r;
		}
	}
	b.keep[ h ] = r.outcome == RMQ_KEEP ? 1 : 0;
}

}	// namespace

int seqcheck_waves( int image_bytes, int frames )
{
	const int	room = RMQ_LDS_BYTES - RMQ_LDS_TABLES - image_bytes, wave = rmq_wave_bytes( frames );
	const int	n = room < wave ? 0 : room / wave;
	return n > RMQ_MAX_WAVES ? RMQ_MAX_WAVES : n;
}

hipError_t seqcheck_records( const SeqBatch &b, hipStream_t s )
{
	if( b.n <= 0 )
		return hipSuccess;
	const int	waves = seqcheck_waves( b.image_bytes, b.frames );
	if( waves < 1 || b.image_bytes % 8 != 0 || b.image_bytes < int( sizeof( RmqImage ) ) || b.frames < 0 || b.stride < 1 )
		return hipErrorInvalidValue;
	const int	block = waves * 64;
	const size_t	lds = size_t( b.image_bytes ) + RMQ_LDS_TABLES + size_t( waves ) * size_t( rmq_wave_bytes( b.frames ) );
	hipLaunchKernelGGL( rma_seqcheck_kernel, dim3( unsigned( ( b.n + block - 1 ) / block ) ), dim3( unsigned( block ) ), lds, s, b );
	return hipGetLastError();
}

hipError_t seqcheck_kernel_attributes( int *private_bytes, int *static_lds, int *regs )
{
	hipFuncAttributes	a;
	const hipError_t	e = hipFuncGetAttributes( &a, reinterpret_cast<const void *>( rma_seqcheck_kernel ) );
	if( e == hipSuccess ){
		*private_bytes = int( a.localSizeBytes );
		*static_lds = int( a.sharedSizeBytes );
		*regs = a.numRegs;
	}
	return e;
}

}	// namespace rma
