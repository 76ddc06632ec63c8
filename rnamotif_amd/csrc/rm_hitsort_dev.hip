// rm_hitsort_dev.hip -- see rm_hitsort_dev.h
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "rm_hitsort_dev.h"

namespace rma {

namespace {

struct Widths { int seq, pos, rank, ord; };

// n: the records the launch is sized for.  With d_count (the tail enqueued ahead of the count, rm_tail_plan.h) the records are
// min( *d_count, n ) and the slots behind them get a key that sorts last: the sort is stable and the records have the lower
// slots, so a record whose own key is all ones stays in front of the padding.
// The flag is raised by storing this run's number (DevHitSort::epoch, never 0, never used twice): nothing has to clear it.
__global__ void __launch_bounds__( 256 )
hit_keys_kernel( const int32_t *hits, long long n, const unsigned long long *d_count, int stride, Widths w, unsigned long long *keys, unsigned *vals,
	unsigned long long *flag, unsigned long long epoch )
{
	__builtin_amdgcn_s_setprio( 3 );	// (behind a drain kernel on its stream it runs beside another scanner's search kernel)
	const long long	i = blockIdx.x * 256ll + threadIdx.x;
	if( i >= n )
		return;
	if( d_count != nullptr && ( unsigned long long )i >= *d_count ){
		keys[ i ] = ~0ull;
		vals[ i ] = unsigned( i );
		return;
	}
	const int32_t	*x = hits + i * stride;
	const unsigned	s = unsigned( x[ 0 ] ), c = unsigned( x[ 1 ] ) & 1u, p = unsigned( x[ 2 ] ), r = unsigned( x[ 3 ] ), o = unsigned( x[ 4 ] );
	// (every width is below 32)
	if( ( s >> w.seq ) | ( p >> w.pos ) | ( r >> w.rank ) | ( o >> w.ord ) )
		atomicMax( flag, epoch );
	unsigned long long	k = ( ( unsigned long long )s << 1 ) | c;
	k = ( k << w.pos ) | p;
	k = ( k << w.rank ) | r;
	k = ( k << w.ord ) | o;
	keys[ i ] = k;
	vals[ i ] = unsigned( i );
}

// The sort of a few thousand pairs without the library: the pairs in front of a pair -- those with a lower key, and of those
// with the same key the ones in lower slots, which is the stable order -- are counted by RANK_PARTS neighbouring lanes, each
// over every RANK_PARTS-th key, and key and slot stored at that rank.  n^2 comparisons of keys that every workgroup stages
// through 8 KB of LDS, 1024 at a time; one kernel where the library takes six at the 7 296 pairs a tail is planned for after
// scans of 5 837 records (a block sort of 22 us and five merge passes of 5 us each: DESIGN.md 6), in workgroups of four
// waves that find room on a CU beside another scanner's search kernel -- which one workgroup sorting all pairs in LDS would
// not (96 KB; the search kernel's plan leaves a CU 33 KB and a wave per SIMD).
#define RANK_CHUNK	1024
#define RANK_PARTS	8
__global__ void __launch_bounds__( 256 )
hit_rank_kernel( const unsigned long long * __restrict__ keys, int n, unsigned long long * __restrict__ skeys, unsigned * __restrict__ perm )
{
	__builtin_amdgcn_s_setprio( 3 );
	__shared__ unsigned long long	s[ RANK_CHUNK ];
	const int	part = threadIdx.x % RANK_PARTS;
	const int	i = blockIdx.x * ( 256 / RANK_PARTS ) + threadIdx.x / RANK_PARTS;
	const unsigned long long	k = i < n ? keys[ i ] : 0;
	int	r = 0;
	for( int base = 0; base < n; base += RANK_CHUNK ){
		__syncthreads();
		for( int j = threadIdx.x; j < RANK_CHUNK; j += 256 )
			s[ j ] = base + j < n ? keys[ base + j ] : ~0ull;
		__syncthreads();
		const int	m = min( RANK_CHUNK, n - base );
		// (the pairs of this chunk in slots below i: equal keys count; from slot i on: lower keys only)
		const int	below = min( max( i - base, 0 ), m );
		int	j = part;
#pragma unroll 4
		for( ; j < below; j += RANK_PARTS )
			r += s[ j ] <= k;
#pragma unroll 4
		for( ; j < m; j += RANK_PARTS )
			r += s[ j ] < k;
	}
	for( int d = 1; d < RANK_PARTS; d <<= 1 )
		r += __shfl_xor( r, d );
	if( part == 0 && i < n ){
		skeys[ r ] = k;
		perm[ r ] = unsigned( i );
	}
}

// a wave per record of the ordered stream; the order word becomes the record's distance from the
// first record of its (entry, strand, start, rank) group, found by bisection in the sorted keys.
// With d_count the waves past min( *d_count, n ) leave at once; with h_out (page-locked memory the
// device writes to) every record is stored there as well: the copy back without a copy of its own.
__global__ void __launch_bounds__( 256 )
hit_gather_kernel( const int32_t *hits, const unsigned *perm, const unsigned long long *skeys, int w_ord,
	long long n, const unsigned long long *d_count, int stride, int32_t *out, int32_t *h_out )
{
	__builtin_amdgcn_s_setprio( 3 );
	const long long	i = blockIdx.x * 4ll + ( threadIdx.x >> 6 );
	if( i >= n || ( d_count != nullptr && ( unsigned long long )i >= *d_count ) )
		return;
	const int32_t	*x = hits + ( long long )perm[ i ] * stride;
	int32_t	*o = out + i * stride;
	for( int w = threadIdx.x & 63; w < stride; w += 64 ){
		int32_t	v = x[ w ];
		if( w == 4 ){
			const unsigned long long	g = skeys[ i ] >> w_ord;
			long long	lo = 0, hi = i;
			while( lo < hi ){
				const long long	mid = ( lo + hi ) >> 1;
				if( ( skeys[ mid ] >> w_ord ) < g )
					lo = mid + 1;
				else
					hi = mid;
			}
			v = int32_t( i - lo );
		}
		o[ w ] = v;
		if( h_out != nullptr )
			h_out[ i * stride + w ] = v;
	}
}

__global__ void __launch_bounds__( 256 )
hit_relabel_kernel( int32_t *hits, long long n, int stride, const int32_t *index, int n_index )
{
	const long long	i = blockIdx.x * 256ll + threadIdx.x;
	if( i >= n )
		return;
	const int32_t	e = hits[ i * stride ];
	if( e >= 0 && e < n_index )
		hits[ i * stride ] = index[ e ];
}

}	// namespace

hipError_t relabel_entries( int32_t *d_hits, int64_t n, int stride, const int32_t *d_index, int32_t n_index, hipStream_t s )
{
	if( n <= 0 )
		return hipSuccess;
	hipLaunchKernelGGL( hit_relabel_kernel, dim3( unsigned( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, s,
		d_hits, ( long long )n, stride, d_index, int( n_index ) );
	return hipGetLastError();
}

void DevHitSort::release()
{
	for( DevMem *m : { &keys[ 0 ], &keys[ 1 ], &vals[ 0 ], &vals[ 1 ], &tmp, &out, &flag } )
		m->reset();
	cap = 0;
}

// (all or nothing: a caller that goes on without the ordering -- rma_scanner_create -- finds cap 0, not a part of it)
hipError_t DevHitSort::reserve( int64_t want, int stride_ )
{
	if( want <= cap && stride_ == stride )
		return hipSuccess;
	release();
	const size_t	n = size_t( want );
	size_t	bytes = 0;
	const unsigned long long	epoch_none = 0;
	hipError_t	e = hipSuccess;
	for( int i = 0; i < 2 && e == hipSuccess; i++ )
		if( ( e = keys[ i ].exact( n * sizeof( unsigned long long ) ) ) == hipSuccess )
			e = vals[ i ].exact( n * sizeof( unsigned ) );
	if( e == hipSuccess )
		e = out.exact( n * stride_ * sizeof( int32_t ) );
	if( e == hipSuccess )
		e = flag.exact( sizeof( unsigned long long ) );
	if( e == hipSuccess )
		e = hipMemcpy( flag.as<void>(), &epoch_none, sizeof( epoch_none ), hipMemcpyHostToDevice );	// (once: a run raises it to its own number)
	if( e == hipSuccess )
		e = rocprim::radix_sort_pairs( nullptr, bytes, keys[ 0 ].as<unsigned long long>(), keys[ 1 ].as<unsigned long long>(),
			vals[ 0 ].as<unsigned>(), vals[ 1 ].as<unsigned>(), n, 0u, 64u );
	if( e == hipSuccess )
		e = tmp.exact( bytes != 0 ? bytes : 16 );
	if( e != hipSuccess ){
		release();
		return e;
	}
	cap = want;
	stride = stride_;
	return hipSuccess;
}

// the library's work area for a sort of n pairs: before anything that reads it is enqueued (a regrow waits for the stream)
hipError_t DevHitSort::plan( int64_t n, hipStream_t s )
{
	if( n <= 0 || n > cap || n > int64_t( 0x7fffffff ) )
		return hipErrorInvalidValue;
	if( n <= RANK_SORT_MAX )
		return hipSuccess;	// (the counting kernel: no work area)
	hipError_t	e;
	size_t	bytes = 0;
	if( ( e = rocprim::radix_sort_pairs( nullptr, bytes, keys[ 0 ].as<unsigned long long>(), keys[ 1 ].as<unsigned long long>(),
			vals[ 0 ].as<unsigned>(), vals[ 1 ].as<unsigned>(), size_t( n ), 0u, 64u, s ) ) != hipSuccess ) return e;
	if( bytes > tmp.bytes() ){
		// (the library picks its algorithm by size: what a small sort needs is not bounded by the largest one's)
		if( ( e = hipStreamSynchronize( s ) ) != hipSuccess ) return e;
		if( ( e = tmp.exact( bytes ) ) != hipSuccess ) return e;
	}
	return hipSuccess;
}

hipError_t DevHitSort::run( const int32_t *d_hits, int64_t n, int w_seq, int w_pos, int w_rank, hipStream_t s )
{
	const hipError_t	e = plan( n, s );
	return e != hipSuccess ? e : run( d_hits, n, nullptr, d_flag(), nullptr, w_seq, w_pos, w_rank, s );
}

hipError_t DevHitSort::run( const int32_t *d_hits, int64_t n, const unsigned long long *d_count, unsigned long long *d_flag_word, int32_t *h_out,
	int w_seq, int w_pos, int w_rank, hipStream_t s )
{
	if( n <= 0 || n > cap || n > int64_t( 0x7fffffff ) )
		return hipErrorInvalidValue;
	Widths	w{ w_seq, w_pos, w_rank, w_ord };
	if( w.seq > 31 || w.pos > 31 || w.rank > 31 )
		return hipErrorInvalidValue;
	if( w.seq + 1 + w.pos + w.rank + w.ord > 64 )
		w.ord = 64 - ( w.seq + 1 + w.pos + w.rank );
	if( w.ord > 31 )
		w.ord = 31;
	if( w.ord < 4 )
		return hipErrorInvalidValue;
	hipError_t	e;
	unsigned long long	*k0 = keys[ 0 ].as<unsigned long long>(), *k1 = keys[ 1 ].as<unsigned long long>();
	unsigned	*v0 = vals[ 0 ].as<unsigned>(), *v1 = vals[ 1 ].as<unsigned>();
	epoch++;
	hipLaunchKernelGGL( hit_keys_kernel, dim3( unsigned( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, s,
		d_hits, ( long long )n, d_count, stride, w, k0, v0, d_flag_word, epoch );
	if( ( e = hipGetLastError() ) != hipSuccess ) return e;
	// All 64 bits of the key, whatever the fields in use: the library picks its kernels by the bit range,
	// and a range that changes with the database means kernels that are loaded in the middle of a search
	// (11 ms in the first batch, measured) instead of by the scanner's warm-up.  The extra passes over a
	// few thousand keys cost microseconds.
	const unsigned	bits = 64u;
	size_t	bytes = tmp.bytes();
	if( n <= RANK_SORT_MAX ){
		hipLaunchKernelGGL( hit_rank_kernel, dim3( unsigned( ( n * RANK_PARTS + 255 ) / 256 ) ), dim3( 256 ), 0, s, k0, int( n ), k1, v1 );
		if( ( e = hipGetLastError() ) != hipSuccess ) return e;
	}else
	if( ( e = rocprim::radix_sort_pairs( tmp.as<void>(), bytes, k0, k1, v0, v1, size_t( n ), 0u, bits, s ) ) != hipSuccess ) return e;
	hipLaunchKernelGGL( hit_gather_kernel, dim3( unsigned( ( n + 3 ) / 4 ) ), dim3( 256 ), 0, s,
		d_hits, v1, k1, w.ord, ( long long )n, d_count, stride, d_out(), h_out );
	return hipGetLastError();
}

}	// namespace rma
