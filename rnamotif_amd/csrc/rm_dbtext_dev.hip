// rm_dbtext_dev.hip -- see rm_dbtext_dev.h and, for the rule, rm_dbtext.h
//
// Every kernel works in whole waves of 64 lanes: what a wave decides it decides for all its lanes, so that the lane
// sums and scans below always see 64 lanes.  No LDS but what the cross-lane moves use.
#include <algorithm>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "rm_dbtext_dev.h"

namespace rma {

namespace {

constexpr int	DT_BLOCK = 256;
constexpr int	DT_WAVES = DT_BLOCK / 64;
constexpr int	DT_GROUPS = 4;		// groups of 64 slots a wave of the fill takes one after the other (4 KB of text)

__device__ inline int wave_sum( int v )
{
#pragma unroll
	for( int o = 32; o > 0; o >>= 1 )
		v += __shfl_xor( v, o );
	return v;
}

// the sum over the lanes below this one
__device__ inline int wave_exclusive( int v, int lane )
{
	int	x = v;
#pragma unroll
	for( int o = 1; o < 64; o <<= 1 ){
		const int	u = __shfl_up( x, o );
		if( lane >= o )
			x += u;
	}
	return x - v;
}

// G( W ): the mask bits set in words [ 0, W ), 0 <= W <= n_mask -- the directory's count for W's run, and the words
// of the run before W a lane each.  W is the wave's.
__device__ inline long long wave_rank( const DbTextArgs &a, long long W, int lane )
{
	const long long	i = dbtext_run_first( W ) + lane;
	const int	c = i < W ? __popc( a.amask[ i ] ) : 0;
	return ( long long )a.dir[ dbtext_run( W ) ] + wave_sum( c );
}

// a wave a run: lane l counts word 64 r + l
__global__ void __launch_bounds__( DT_BLOCK )
rma_dbtext_count_kernel( DbTextArgs a, long long runs )
{
	const long long	w = blockIdx.x * ( long long )DT_BLOCK + threadIdx.x;
	const long long	r = w / DT_RUN_WORDS;
	if( r >= runs )
		return;
	const int	c = wave_sum( w < a.n_mask ? __popc( a.amask[ w ] ) : 0 );
	if( ( threadIdx.x & 63 ) == 0 )
		a.dir[ r ] = uint64_t( c );
}

// a wave an entry: the bits its mask has set in [ 0, slen ) are G( its end ) - G( its first word )
__global__ void __launch_bounds__( DT_BLOCK )
rma_dbtext_entry_kernel( DbTextArgs a )
{
	const int	lane = threadIdx.x & 63;
	const long long	e = blockIdx.x * ( long long )DT_WAVES + ( threadIdx.x >> 6 );
	if( e >= a.n )
		return;
	const long long	w0 = a.base_off[ e ] / 32;
	const int32_t	slen = a.slen[ e ];
	const long long	w1 = w0 + ( slen >> 5 );
	const int	b = slen & 31;
	const long long	g0 = wave_rank( a, w0, lane );
	const long long	g1 = wave_rank( a, w1, lane ) + ( b != 0 ? __popc( a.amask[ w1 ] & ( ( 1u << b ) - 1u ) ) : 0 );
	if( lane != 0 || a.exc == nullptr )
		return;
	a.exc_base[ e ] = a.exc_off[ e ] - g0;
	if( g1 - g0 != a.exc_off[ e + 1 ] - a.exc_off[ e ] )
		atomicMin( a.bad, dbtext_bad_word( int32_t( e ), DT_BAD_COUNT, uint32_t( g1 - g0 ) ) );
}

// a lane an exception byte
__global__ void __launch_bounds__( DT_BLOCK )
rma_dbtext_letter_kernel( DbTextArgs a )
{
	const long long	k = blockIdx.x * ( long long )DT_BLOCK + threadIdx.x;
	if( k >= a.n_exc )
		return;
	const unsigned char	c = static_cast<unsigned char>( a.exc[ k ] );
	if( dbtext_exc_letter( c ) )
		return;
	// (the entry whose exceptions hold byte k: the last one that starts at or before it)
	const int32_t	e = dbtext_entry_at( a.exc_off, 0, a.n, k ) - 1;
	atomicMin( a.bad, dbtext_bad_word( e, DT_BAD_LETTER, c ) );
}

// A lane a slot: one code word in, 16 letters out as one 16-byte store.  A wave takes DT_GROUPS groups of 64
// consecutive slots.  A group inside one entry -- all of them but those at the entries' seams, when the entries are
// long -- finds its ranks with one G() for its first mask word and a lane scan; a group over several entries gives
// each of its lanes that has masked bases a G() of its own, the wave working for one lane at a time.  A wave whose
// groups all lie in one entry looks the entry up once and has the loads of all its groups in flight together.
__device__ inline void store_slot( const DbTextArgs &a, long long t, const uint64_t out[ 2 ] )
{
	*reinterpret_cast<uint4 *>( a.text + DT_SLOT * t ) = make_uint4( uint32_t( out[ 0 ] ), uint32_t( out[ 0 ] >> 32 ),
		uint32_t( out[ 1 ] ), uint32_t( out[ 1 ] >> 32 ) );
}

// The lane's slot t of a group of 64 inside one entry: slot cw of the entry, whose first mask word is w_e; code and mw
// its code word and mask word (live: t is a slot of the text; lane 0's is).
__device__ inline void fill_in_entry( const DbTextArgs &a, long long exc_base, long long w_e, int32_t slen, long long cw, long long t,
	bool live, uint32_t code, uint32_t mw, int lane )
{
	const uint32_t	m = live ? dbtext_slot_mask( mw, cw, slen ) : 0u;
	uint64_t	out[ 2 ];
	dbtext_slot_plain( code, m, dbtext_slot_tail( cw, slen ), out );
	if( a.exc != nullptr && __ballot( m != 0u ) != 0ull ){
		// (lane 0's mask word is the group's first, the lanes' slots follow each other)
		const long long	W0 = w_e + ( __shfl( cw, 0 ) >> 1 );
		const int	below0 = __shfl( __popc( dbtext_below_slot( mw, cw ) ), 0 );
		const long long	idx = dbtext_exc_index( exc_base, wave_rank( a, W0, lane ), wave_exclusive( __popc( m ), lane ), below0 );
		if( m != 0u )
			dbtext_slot_patch( m, a.exc, idx, a.n_exc, out );
	}
	if( live )
		store_slot( a, t, out );
}

__global__ void __launch_bounds__( DT_BLOCK )
rma_dbtext_fill_kernel( DbTextArgs a )
{
	const int	lane = threadIdx.x & 63;
	// (the wave's number in a scalar register: what depends on it alone is loaded once a wave)
	const long long	wave = blockIdx.x * ( long long )DT_WAVES + __builtin_amdgcn_readfirstlane( int( threadIdx.x >> 6 ) );
	const long long	slots = a.text_bytes / DT_SLOT;
	const long long	s0 = wave * DT_GROUPS * 64;
	if( s0 >= slots )
		return;
	const long long	sl = ( s0 + DT_GROUPS * 64 < slots ? s0 + DT_GROUPS * 64 : slots ) - 1;
	int32_t	e_prev = dbtext_entry_at( a.text_start, 0, a.n, DT_SLOT * s0 ) - 1;	// the entry of the wave's first slot
	long long	prev_lo = a.text_start[ e_prev ];				// ... and its bytes of the text
	long long	prev_hi = e_prev + 1 < a.n ? a.text_start[ e_prev + 1 ] : a.text_bytes;
	if( DT_SLOT * sl < prev_hi ){
		// all the wave's slots in one entry: the words of its groups fetched side by side
		const long long	base_off = a.base_off[ e_prev ], cw0 = s0 - prev_lo / DT_SLOT;
		const int32_t	slen = a.slen[ e_prev ];
		const long long	exc_base = a.exc != nullptr ? a.exc_base[ e_prev ] : 0;
		const uint32_t	*codes = a.codes + base_off / 16, *amask = a.amask + base_off / 32;
		uint32_t	code[ DT_GROUPS ], mw[ DT_GROUPS ];
#pragma unroll
		for( int it = 0; it < DT_GROUPS; it++ ){
			const long long	cw = cw0 + it * 64 + lane;
			const bool	live = s0 + it * 64 + lane <= sl;
			code[ it ] = live ? codes[ cw ] : 0u;
			mw[ it ] = live ? amask[ cw >> 1 ] : 0u;
		}
#pragma unroll
		for( int it = 0; it < DT_GROUPS; it++ )
			if( s0 + it * 64 <= sl )
				fill_in_entry( a, exc_base, base_off / 32, slen, cw0 + it * 64 + lane, s0 + it * 64 + lane, s0 + it * 64 + lane <= sl,
					code[ it ], mw[ it ], lane );
		return;
	}
	for( int it = 0; it < DT_GROUPS; it++ ){
		const long long	t0 = ( wave * DT_GROUPS + it ) * 64;
		if( t0 >= slots )
			break;
		const long long	t = t0 + lane, tl = t0 + 63 < slots ? t0 + 63 : slots - 1;
		const bool	live = t < slots;
		int32_t	e0, e1;
		if( DT_SLOT * t0 >= prev_lo && DT_SLOT * tl < prev_hi )
			e0 = e1 = e_prev;
		else{
			e0 = dbtext_entry_at( a.text_start, e_prev, a.n, DT_SLOT * t0 ) - 1;
			e1 = dbtext_entry_at( a.text_start, e0, a.n, DT_SLOT * tl ) - 1;
			e_prev = e1;
			prev_lo = a.text_start[ e1 ];
			prev_hi = e1 + 1 < a.n ? a.text_start[ e1 + 1 ] : a.text_bytes;
		}
		const bool	one = e0 == e1;
		const int32_t	e = one || !live ? e0 : dbtext_entry_at( a.text_start, e0, e1 + 1, DT_SLOT * t ) - 1;
		// the slot's code word, its mask word and what of them are bases
		const long long	cw = live ? t - a.text_start[ e ] / DT_SLOT : 0;
		const long long	base_off = a.base_off[ e ];
		const int32_t	slen = a.slen[ e ];
		const long long	W = base_off / 32 + ( cw >> 1 );
		const uint32_t	code = live ? a.codes[ base_off / 16 + cw ] : 0u;
		const uint32_t	mw = live ? a.amask[ W ] : 0u;
		if( one ){
			fill_in_entry( a, a.exc != nullptr ? a.exc_base[ e ] : 0, base_off / 32, slen, cw, t, live, code, mw, lane );
			continue;
		}
		const uint32_t	m = live ? dbtext_slot_mask( mw, cw, slen ) : 0u;
		uint64_t	out[ 2 ];
		dbtext_slot_plain( code, m, dbtext_slot_tail( cw, slen ), out );
		if( a.exc != nullptr && __ballot( m != 0u ) != 0ull ){
			long long	idx = 0;
			unsigned long long	todo = __ballot( m != 0u );
			while( todo != 0ull ){
				const int	src = __ffsll( ( long long )todo ) - 1;
				todo &= todo - 1;
				const long long	g = wave_rank( a, __shfl( W, src ), lane );
				if( lane == src )
					idx = dbtext_exc_index( a.exc_base[ e ], g, 0, __popc( dbtext_below_slot( mw, cw ) ) );
			}
			if( m != 0u )
				dbtext_slot_patch( m, a.exc, idx, a.n_exc, out );
		}
		if( live )
			store_slot( a, t, out );
	}
}

}	// namespace

hipError_t dbtext_directory( const DbTextArgs &a, void *tmp, size_t *tmp_bytes, hipStream_t s )
{
	const long long	runs = dbtext_dir_runs( a.n_mask );
	if( tmp == nullptr )
		return rocprim::exclusive_scan( nullptr, *tmp_bytes, a.dir, a.dir, uint64_t( 0 ), size_t( runs ), rocprim::plus<uint64_t>(), s );
	hipLaunchKernelGGL( rma_dbtext_count_kernel, dim3( unsigned( ( runs * DT_RUN_WORDS + DT_BLOCK - 1 ) / DT_BLOCK ) ), dim3( DT_BLOCK ), 0, s, a, runs );
	hipError_t	e = hipGetLastError();
	if( e != hipSuccess )
		return e;
	return rocprim::exclusive_scan( tmp, *tmp_bytes, a.dir, a.dir, uint64_t( 0 ), size_t( runs ), rocprim::plus<uint64_t>(), s );
}

hipError_t dbtext_check( const DbTextArgs &a, hipStream_t s )
{
	if( a.n > 0 ){
		hipLaunchKernelGGL( rma_dbtext_entry_kernel, dim3( unsigned( ( ( long long )a.n + DT_WAVES - 1 ) / DT_WAVES ) ), dim3( DT_BLOCK ), 0, s, a );
		hipError_t	e = hipGetLastError();
		if( e != hipSuccess )
			return e;
	}
	if( a.exc != nullptr && a.n_exc > 0 ){
		hipLaunchKernelGGL( rma_dbtext_letter_kernel, dim3( unsigned( ( a.n_exc + DT_BLOCK - 1 ) / DT_BLOCK ) ), dim3( DT_BLOCK ), 0, s, a );
		return hipGetLastError();
	}
	return hipSuccess;
}

hipError_t dbtext_fill( const DbTextArgs &a, hipStream_t s )
{
	const long long	slots = a.text_bytes / DT_SLOT;
	if( slots <= 0 || a.n <= 0 )
		return hipSuccess;
	const long long	per_block = 64ll * DT_GROUPS * DT_WAVES, blocks = ( slots + per_block - 1 ) / per_block;
	if( blocks > 0x7fffffffll )
		return hipErrorInvalidValue;
	hipLaunchKernelGGL( rma_dbtext_fill_kernel, dim3( unsigned( blocks ) ), dim3( DT_BLOCK ), 0, s, a );
	return hipGetLastError();
}

}	// namespace rma
