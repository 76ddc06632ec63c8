// rm_prune_dev.hip -- see rm_prune_dev.h
#include <algorithm>
#include <hip/hip_runtime.h>
#include "rm_prune_dev.h"

namespace rma {

namespace {

constexpr int	PRUNE_REZIP_GRID = 1 << 16;	// workgroups of the rezip kernel at most; more blocks go grid-stride
static_assert( sizeof( PruneJudged ) == 12, "the judged elements are copied to LDS word by word" );

struct MaxOp {
	static __device__ long long	none() { return -1; }
	static __device__ long long	join( long long a, long long b ) { return a > b ? a : b; }
};
struct SumOp {
	static __device__ long long	none() { return 0; }
	static __device__ long long	join( long long a, long long b ) { return a + b; }
};

// the inclusive scan of one value per thread of a workgroup of PRUNE_WG, through sh[ PRUNE_WG ]
template<class Op> __device__ long long wg_scan( long long v, long long *sh )
{
	const int	t = threadIdx.x;
	sh[ t ] = v;
	__syncthreads();
	for( int d = 1; d < PRUNE_WG; d <<= 1 ){
		const long long	x = t >= d ? sh[ t - d ] : Op::none();
		__syncthreads();
		sh[ t ] = Op::join( sh[ t ], x );
		__syncthreads();
	}
	return sh[ t ];
}

// the name group of record h's entry; -1 for an entry outside the database (the call fails on such a record)
__device__ int32_t group_of( const int32_t *hits, long long h, int stride, int n_seq, const int32_t *groups )
{
	const int32_t	e = hits[ h * stride ];
	if( e < 0 || e >= n_seq )
		return -1;
	return groups != nullptr ? groups[ e ] : e;
}

__global__ void __launch_bounds__( PRUNE_WG )
rma_prune_keys_kernel( const int32_t *hits, long long n, int stride, HitWinShape shape, int row, const int32_t *slen, int n_seq, PruneDev d )
{
	__shared__ long long	sh[ PRUNE_WG ];
	const long long	h = blockIdx.x * ( long long )PRUNE_WG + threadIdx.x;
	long long	mine = -1;
	if( h < n ){
		const int32_t	*w = hits + h * stride;
		int32_t	lo, hi, css[ 3 ] = { 0, 0, 0 };
		int	which;
		if( hitwin_span( w, shape, n_seq, slen, &lo, &hi, &which ) != HW_OK )
			atomicMin( d.bad, static_cast<unsigned long long>( h ) );
		else
			prune_keys( w, *d.tab, shape, slen[ w[ 0 ] ], css, d.rows + h * row );
		const int	first = h == 0 || group_of( hits, h, stride, n_seq, d.groups ) != group_of( hits, h - 1, stride, n_seq, d.groups );
		*reinterpret_cast<int4 *>( d.hdr + 4 * h ) = make_int4( css[ 0 ], css[ 1 ], css[ 2 ], first );
		if( first )
			mine = h;
	}
	const long long	all = wg_scan<MaxOp>( mine, sh );
	if( threadIdx.x == PRUNE_WG - 1 )
		d.part[ blockIdx.x ] = all;
}

// one workgroup: out_x[ i ] = in[ 0 ] .. in[ i - 1 ] joined, *total (if asked for) all of them
template<class Op> __global__ void __launch_bounds__( PRUNE_WG )
rma_prune_part_kernel( const long long *in, long long *out_x, long long parts, long long *total )
{
	__shared__ long long	sh[ PRUNE_WG ];
	const int	t = threadIdx.x;
	const long long	per = ( parts + PRUNE_WG - 1 ) / PRUNE_WG, a = t * per < parts ? t * per : parts, b = a + per < parts ? a + per : parts;
	long long	acc = Op::none();
	for( long long i = a; i < b; i++ )
		acc = Op::join( acc, in[ i ] );
	sh[ t ] = acc;
	__syncthreads();
	if( t == 0 ){
		long long	run = Op::none();
		for( int k = 0; k < PRUNE_WG; k++ ){
			const long long	x = sh[ k ];
			sh[ k ] = run;
			run = Op::join( run, x );
		}
		if( total != nullptr )
			*total = run;
	}
	__syncthreads();
	acc = sh[ t ];
	for( long long i = a; i < b; i++ ){
		out_x[ i ] = acc;
		acc = Op::join( acc, in[ i ] );
	}
}

__global__ void __launch_bounds__( PRUNE_WG )
rma_prune_starts_kernel( long long n, PruneDev d )
{
	__shared__ long long	sh[ PRUNE_WG ];
	const long long	h = blockIdx.x * ( long long )PRUNE_WG + threadIdx.x;
	const long long	mine = h < n && d.hdr[ 4 * h + 3 ] ? h : -1;
	// (record 0 is a run start: every record has one at or before it)
	const long long	run = MaxOp::join( wg_scan<MaxOp>( mine, sh ), d.part_x[ blockIdx.x ] );
	const int	bf = h < n && ( h - run ) % PRUNE_BLOCK == 0;
	if( h < n )
		d.bflag[ h ] = uint8_t( bf );
	const int	count = __syncthreads_count( bf );
	if( threadIdx.x == 0 )
		d.part[ blockIdx.x ] = count;
}

__global__ void __launch_bounds__( PRUNE_WG )
rma_prune_list_kernel( long long n, PruneDev d )
{
	__shared__ long long	sh[ PRUNE_WG ];
	const long long	h = blockIdx.x * ( long long )PRUNE_WG + threadIdx.x;
	const int	bf = h < n ? d.bflag[ h ] : 0;
	const long long	before = wg_scan<SumOp>( bf, sh ) - bf;
	if( bf )
		d.blocks[ d.part_x[ blockIdx.x ] + before ] = h;
}

// A wave per block, blocks taken grid-stride (rm_prune_dev.h has the plan).  Every branch and loop bound below is
// the same on all lanes of the wave, so the ballots and barriers run with the whole wave there.  A block has 1 to
// PRUNE_BLOCK records by the way the list was made: consecutive block starts are at most that far apart.
__global__ void __launch_bounds__( 64 )
rma_prune_rezip_kernel( long long n, int row, PruneDev d, long long n_blocks, uint8_t *keep )
{
	__shared__ PruneJudged	judged[ RMA_MAX_ELEMS ];
	__shared__ int32_t	st[ PRUNE_BLOCK ], sp[ PRUNE_BLOCK ];
	__shared__ uint8_t	kp[ PRUNE_BLOCK ], cm[ PRUNE_BLOCK ];
	const int	lane = threadIdx.x;
	const int	nj = d.tab->n_judged;
	{
		const int32_t	*g = reinterpret_cast<const int32_t *>( d.tab->judged );
		int32_t	*s = reinterpret_cast<int32_t *>( judged );
		for( int k = lane; k < 3 * nj; k += 64 )
			s[ k ] = g[ k ];
	}
	for( long long k = blockIdx.x; k < n_blocks; k += gridDim.x ){
		const long long	s = d.blocks[ k ], e = k + 1 < n_blocks ? d.blocks[ k + 1 ] : n;
		const int	m = int( e - s < PRUNE_BLOCK ? e - s : PRUNE_BLOCK );
		__syncthreads();
		int	fc = m;
		for( int c0 = 0; c0 < m; c0 += 64 ){
			const int	i = c0 + lane;
			int	comp = 0;
			if( i < m ){
				const int4	x = *reinterpret_cast<const int4 *>( d.hdr + 4 * ( s + i ) );
				comp = x.x;
				st[ i ] = x.y;
				sp[ i ] = x.z;
				cm[ i ] = uint8_t( comp );
				kp[ i ] = 1;
			}
			const unsigned long long	any = __ballot( comp != 0 );
			if( any != 0 && fc == m )
				fc = c0 + __builtin_ctzll( any );
		}
		__syncthreads();
		for( int sec = 0; sec < 2; sec++ ){
			const int	to = sec ? m : fc;
			for( int lb = sec ? fc : 0; lb < to; ){
				// the next leader: the first record behind lb that leaves lb's span
				const int32_t	gs = st[ lb ], ge = sp[ lb ];
				int	b = to;
				for( int c0 = lb + 1; c0 < to; c0 += 64 ){
					const int	i = c0 + lane;
					const unsigned long long	out = __ballot( i < to && prune_leaves( sec != 0, st[ i < to ? i : lb ], sp[ i < to ? i : lb ], gs, ge ) );
					if( out != 0 ){
						b = c0 + __builtin_ctzll( out );
						break;
					}
				}
				// rezip() of [ lb, b )
				for( int bb = b - 1; bb > lb; bb-- ){
					if( !kp[ bb ] )
						continue;
					const int32_t	*ra = d.rows + ( s + bb ) * row;
					const int	comp = cm[ bb ];
					for( int top = bb - 1; top >= lb; top -= 64 ){
						const int	b1 = top - lane;
						int	r = PR_SAME;
						if( b1 >= lb && kp[ b1 ] )
							r = prune_relation( judged, nj, comp, ra, d.rows + ( s + b1 ) * row );
						const unsigned long long	left = __ballot( r == PR_LEFT );
						const int	stop_at = left != 0 ? __builtin_ctzll( left ) : 64;	// (lane 0 has the highest b1)
						if( r == PR_DOWN && lane < stop_at )
							kp[ b1 ] = 0;
						if( left != 0 && lane == 0 )
							kp[ bb ] = 0;
						__syncthreads();
						if( left != 0 )
							break;
					}
				}
				lb = b;
			}
		}
		__syncthreads();
		for( int i = lane; i < m; i += 64 )
			keep[ s + i ] = kp[ i ];
	}
}

}	// namespace

hipError_t prune_blocks( const int32_t *d_hits, int64_t n, int stride, const HitWinShape &shape, int row, const int32_t *d_slen,
	int32_t n_seq, const PruneDev &d, hipStream_t s )
{
	if( n <= 0 )
		return hipErrorInvalidValue;
	const long long	parts = prune_parts( n );
	const dim3	grid( static_cast<unsigned>( parts ) ), wg( PRUNE_WG );
	hipLaunchKernelGGL( rma_prune_keys_kernel, grid, wg, 0, s, d_hits, ( long long )n, stride, shape, row, d_slen, int( n_seq ), d );
	hipLaunchKernelGGL( rma_prune_part_kernel<MaxOp>, dim3( 1 ), wg, 0, s, d.part, d.part_x, parts, static_cast<long long *>( nullptr ) );
	hipLaunchKernelGGL( rma_prune_starts_kernel, grid, wg, 0, s, ( long long )n, d );
	hipLaunchKernelGGL( rma_prune_part_kernel<SumOp>, dim3( 1 ), wg, 0, s, d.part, d.part_x, parts, d.n_blocks );
	hipLaunchKernelGGL( rma_prune_list_kernel, grid, wg, 0, s, ( long long )n, d );
	return hipGetLastError();
}

hipError_t prune_rezip( int64_t n, int row, const PruneDev &d, int64_t n_blocks, uint8_t *d_keep, hipStream_t s )
{
	if( n <= 0 || n_blocks <= 0 || n_blocks > n )
		return hipErrorInvalidValue;
	const unsigned	grid = unsigned( std::min<int64_t>( n_blocks, PRUNE_REZIP_GRID ) );
	hipLaunchKernelGGL( rma_prune_rezip_kernel, dim3( grid ), dim3( 64 ), 0, s, ( long long )n, row, d, ( long long )n_blocks, d_keep );
	return hipGetLastError();
}

}	// namespace rma
