// rm_fasta_dev.hip -- see rm_fasta_dev_kernels.h
//
// A chunk is FD_CHUNK bytes counted from the aligned dword the text begins in, so that every load is an
// aligned dword whatever the text's alignment; the bytes of the first and last dword that lie outside
// the text count as bytes that are dropped.  A wave takes a quarter of its chunk, 256 bytes a step: lane l
// holds bytes 4l .. 4l+3.  What a lane needs of the lanes before it comes from three ballots (has a '\n';
// has a '>'; has a '>' after its last '\n'): the state in front of lane l is that of the last lane before
// it with a newline, else the state in front of the step, each joined with the '>' in between.  With its
// state a lane classifies its four bytes (fd_apply_byte); four ballots per class and a popcount of the
// lanes below (mbcnt) give every kept letter its place and every start its entry number.
//
// summarise: each wave sums its sixteen steps for both incoming states (the second only until the two
// agree, after the first newline), the four waves' summaries meet in LDS.  apply: the same pass first,
// the dwords staying in registers, so that every wave learns what the waves before it add (wave offsets
// through LDS); then the steps again with the state, the letter position and the entry number known.
#include <hip/hip_runtime.h>
#include "rm_fasta_dev_kernels.h"

namespace rma {

namespace {

constexpr int	FD_WAVES = FD_THREADS / 64;
constexpr int	FD_STEPS = FD_CHUNK / FD_WAVES / 256;	// steps of 256 bytes per wave
static_assert( FD_CHUNK == FD_WAVES * FD_STEPS * 256, "a chunk is whole steps of every wave" );
static_assert( FD_SCAN_BLOCK == FD_THREADS, "one lane per summary of a scan block" );

struct FdStep {
	uint32_t	keep;		// this lane: bits 0-3 letters kept, 4-7 entries starting, 8-11 definition lines ending
	uint32_t	let_before, st_before;	// letters / starts of the lanes before this one
	int	nlet, nst, out;		// the step's letters and starts, the state behind it
};

__device__ __forceinline__ uint32_t below( unsigned long long m, uint32_t acc )
{
	return __builtin_amdgcn_mbcnt_hi( uint32_t( m >> 32 ), __builtin_amdgcn_mbcnt_lo( uint32_t( m ), acc ) );
}

// x: the lane's dword; vm: which of its bytes are text; in: the state in front of the step (uniform)
__device__ __forceinline__ FdStep fd_wave_step( uint32_t x, uint32_t vm, int in )
{
	unsigned	cls[ 4 ];
	bool	lane_nl = false, lane_gt = false, tail = false;
#pragma unroll
	for( int j = 0; j < 4; j++ ){
		const unsigned	c = ( vm >> j ) & 1u ? fd_class( ( unsigned char )( x >> ( 8 * j ) ) ) : 0u;
		cls[ j ] = c;
		if( c & FD_NL ){
			lane_nl = true;
			tail = false;
		}else if( c & FD_GT )
			lane_gt = tail = true;
	}
	const unsigned long long	NL = __ballot( lane_nl ), GT = __ballot( lane_gt ), TL = __ballot( tail );
	const unsigned	lane = __lane_id();
	const unsigned long long	lt = ( 1ull << lane ) - 1ull;
	int	st;
	if( NL & lt ){
		const int	m = 63 - __clzll( ( long long )( NL & lt ) );
		st = ( ( ( GT & lt ) >> m ) >> 1 ) != 0 || ( ( TL >> m ) & 1ull );
	}else
		st = in | ( ( GT & lt ) != 0 );
	FdStep	r;
	r.keep = 0;
#pragma unroll
	for( int j = 0; j < 4; j++ ){
		const unsigned	k = fd_apply_byte( cls[ j ], &st );
		r.keep |= ( ( k & FD_LETTER ) ? 1u : 0u ) << j | ( ( k & FD_GT ) ? 16u : 0u ) << j | ( ( k & FD_NL ) ? 256u : 0u ) << j;
	}
	if( NL ){
		const int	m = 63 - __clzll( ( long long )NL );
		r.out = ( ( GT >> m ) >> 1 ) != 0 || ( ( TL >> m ) & 1ull );
	}else
		r.out = in | ( GT != 0 );
	r.let_before = r.st_before = 0;
	r.nlet = r.nst = 0;
#pragma unroll
	for( int j = 0; j < 4; j++ ){
		const unsigned long long	L = __ballot( ( r.keep >> j ) & 1u ), S = __ballot( ( r.keep >> ( 4 + j ) ) & 1u );
		r.let_before = below( L, r.let_before );
		r.st_before = below( S, r.st_before );
		r.nlet += __popcll( L );
		r.nst += __popcll( S );
	}
	return r;
}

// The wave's dwords of chunk c, x[ FD_STEPS ], and which of their bytes are text, and its summary.
// words: the aligned dword the text begins in; lead: the text's first byte in it; v_end = lead + text_bytes.
__device__ __forceinline__ FdSummary fd_wave_summary( const uint32_t *words, long long v0, int lead, long long v_end,
	uint32_t ( &x )[ FD_STEPS ], uint32_t ( &vm )[ FD_STEPS ] )
{
	const unsigned	lane = __lane_id();
#pragma unroll
	for( int i = 0; i < FD_STEPS; i++ ){
		const long long	v = v0 + 256 * i + 4 * lane;	// the dword's first byte, counted from words
		uint32_t	m = 0;
#pragma unroll
		for( int j = 0; j < 4; j++ )
			m |= ( v + j >= lead && v + j < v_end ? 1u : 0u ) << j;
		vm[ i ] = m;
		x[ i ] = m ? words[ v >> 2 ] : 0u;
	}
	int	a0 = 0, a1 = 1;
	uint32_t	let0 = 0, let1 = 0, st0 = 0, st1 = 0;
#pragma unroll
	for( int i = 0; i < FD_STEPS; i++ ){
		const FdStep	r0 = fd_wave_step( x[ i ], vm[ i ], a0 );
		if( a1 != a0 ){		// (uniform: the two agree from the first newline on)
			const FdStep	r1 = fd_wave_step( x[ i ], vm[ i ], a1 );
			let1 += r1.nlet;
			st1 += r1.nst;
			a1 = r1.out;
		}else{
			let1 += r0.nlet;
			st1 += r0.nst;
			a1 = r0.out;
		}
		let0 += r0.nlet;
		st0 += r0.nst;
		a0 = r0.out;
	}
	return FdSummary{ { let0, let1 }, { st0, st1 }, uint32_t( a0 ) | uint32_t( a1 ) << 1 };
}

__global__ void __launch_bounds__( FD_THREADS )
rma_fasta_summarise_kernel( const uint32_t *words, int lead, long long v_end, FdSummary *sum )
{
	__shared__ FdSummary	part[ FD_WAVES ];
	const int	wave = threadIdx.x >> 6;
	uint32_t	x[ FD_STEPS ], vm[ FD_STEPS ];
	const long long	v0 = blockIdx.x * ( long long )FD_CHUNK + wave * ( FD_CHUNK / FD_WAVES );
	const FdSummary	mine = fd_wave_summary( words, v0, lead, v_end, x, vm );
	if( ( threadIdx.x & 63 ) == 0 )
		part[ wave ] = mine;
	__syncthreads();
	if( threadIdx.x == 0 ){
		FdSummary	r = part[ 0 ];
		for( int w = 1; w < FD_WAVES; w++ )
			r = fd_compose( r, part[ w ] );
		sum[ blockIdx.x ] = r;
	}
}

// local[ c ]: the chunks of c's block before c, composed; block_sum[ b ]: all of block b's
__global__ void __launch_bounds__( FD_THREADS )
rma_fasta_scan_blocks_kernel( const FdSummary *sum, long long n_chunks, FdSummary *local, FdSummary *block_sum )
{
	__shared__ FdSummary	buf[ 2 ][ FD_SCAN_BLOCK ];
	const int	t = threadIdx.x;
	const long long	c = blockIdx.x * ( long long )FD_SCAN_BLOCK + t;
	buf[ 0 ][ t ] = c < n_chunks ? sum[ c ] : fd_identity<uint32_t>();
	__syncthreads();
	int	cur = 0;
	for( int d = 1; d < FD_SCAN_BLOCK; d <<= 1 ){
		buf[ cur ^ 1 ][ t ] = t >= d ? fd_compose( buf[ cur ][ t - d ], buf[ cur ][ t ] ) : buf[ cur ][ t ];
		cur ^= 1;
		__syncthreads();
	}
	if( c < n_chunks )
		local[ c ] = t > 0 ? buf[ cur ][ t - 1 ] : fd_identity<uint32_t>();
	if( t == FD_SCAN_BLOCK - 1 )
		block_sum[ blockIdx.x ] = buf[ cur ][ t ];
}

// one workgroup: lane t walks a run of blocks, lane 0 the 256 runs, then every lane its run again
__global__ void __launch_bounds__( FD_THREADS )
rma_fasta_scan_top_kernel( const FdSummary *block_sum, long long n_blocks, FdPrefix *block_pre, FdPrefix *totals )
{
	__shared__ FdSummary64	run[ FD_THREADS ];
	__shared__ FdPrefix	pre[ FD_THREADS ];
	const int	t = threadIdx.x;
	const long long	per = ( n_blocks + FD_THREADS - 1 ) / FD_THREADS;
	const long long	b0 = t * per < n_blocks ? t * per : n_blocks, b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
	FdSummary64	r = fd_identity<int64_t>();
	for( long long b = b0; b < b1; b++ )
		r = fd_compose( r, block_sum[ b ] );
	run[ t ] = r;
	__syncthreads();
	if( t == 0 ){
		FdPrefix	p{ 0, 0, 0, 0 };	// the text begins outside a definition line
		for( int k = 0; k < FD_THREADS; k++ ){
			pre[ k ] = p;
			p = fd_advance( p, run[ k ] );
		}
		*totals = p;
	}
	__syncthreads();
	FdPrefix	p = pre[ t ];
	for( long long b = b0; b < b1; b++ ){
		block_pre[ b ] = p;
		p = fd_advance( p, block_sum[ b ] );
	}
}

__global__ void __launch_bounds__( FD_THREADS )
rma_fasta_apply_kernel( const uint32_t *words, int lead, long long v_end, const FdSummary *local, const FdPrefix *block_pre,
	const FdPrefix *totals, uint8_t *clean, long long *gt_off, long long *def_end, long long *first )
{
	__shared__ FdSummary	part[ FD_WAVES ];
	const int	wave = threadIdx.x >> 6;
	const long long	c = blockIdx.x;
	uint32_t	x[ FD_STEPS ], vm[ FD_STEPS ];
	const long long	v0 = c * ( long long )FD_CHUNK + wave * ( FD_CHUNK / FD_WAVES );
	const FdSummary	mine = fd_wave_summary( words, v0, lead, v_end, x, vm );
	if( ( threadIdx.x & 63 ) == 0 )
		part[ wave ] = mine;
	__syncthreads();
	FdPrefix	p = fd_advance( block_pre[ c / FD_SCAN_BLOCK ], local[ c ] );
	for( int w = 0; w < wave; w++ )
		p = fd_advance( p, part[ w ] );
	// (the totals bound every store: text that changes between the launches must not write outside the arrays)
	const long long	n_let = totals->letters, n_st = totals->starts;
	const unsigned	lane = __lane_id();
	int	state = p.state;
	long long	let_at = p.letters, st_at = p.starts;
#pragma unroll
	for( int i = 0; i < FD_STEPS; i++ ){
		const FdStep	r = fd_wave_step( x[ i ], vm[ i ], state );
		if( r.keep ){
			long long	at = let_at + r.let_before, k = st_at + r.st_before;
			const long long	off = v0 + 256 * i + 4 * lane - lead;	// the dword's first byte, from text
#pragma unroll
			for( int j = 0; j < 4; j++ ){
				if( ( r.keep >> j ) & 1u ){
					if( at < n_let )
						clean[ at ] = uint8_t( x[ i ] >> ( 8 * j ) );
					at++;
				}else if( ( r.keep >> ( 4 + j ) ) & 1u ){
					if( k < n_st ){
						gt_off[ k ] = off + j;
						first[ k ] = at;
					}
					k++;
				}else if( ( r.keep >> ( 8 + j ) ) & 1u ){
					if( k >= 1 && k <= n_st )
						def_end[ k - 1 ] = off + j;
				}
			}
		}
		state = r.out;
		let_at += r.nlet;
		st_at += r.nst;
	}
	// a last definition line without its newline ends with the text
	if( c == gridDim.x - 1 && threadIdx.x == 0 && totals->state == 1 && n_st > 0 )
		def_end[ n_st - 1 ] = v_end - lead;
}

__global__ void __launch_bounds__( FD_THREADS )
rma_fasta_headers_kernel( const uint8_t *text, long long text_bytes, const long long *gt_off, const long long *def_end,
	const long long *hdr_off, long long n, uint8_t *out )
{
	const long long	e = blockIdx.x * ( long long )FD_WAVES + ( threadIdx.x >> 6 );
	if( e >= n )
		return;
	const long long	from = gt_off[ e ], to = def_end[ e ] < text_bytes ? def_end[ e ] : text_bytes;
	long long	len = to - from;
	if( from < 0 || len <= 0 )
		return;
	if( len > FD_HEADER_CAP )
		len = FD_HEADER_CAP;
	uint8_t	*dst = out + hdr_off[ e ];
	for( long long i = threadIdx.x & 63; i < len; i += 64 )
		dst[ i ] = text[ from + i ];
}

inline const uint32_t *words_of( const uint8_t *text )
{
	return reinterpret_cast<const uint32_t *>( reinterpret_cast<uintptr_t>( text ) & ~uintptr_t( 3 ) );
}

}	// namespace

hipError_t fasta_index( const uint8_t *text, int64_t text_bytes, FdSummary *d_sum, FdSummary *d_local, FdSummary *d_block_sum,
	FdPrefix *d_block_pre, FdPrefix *d_totals, hipStream_t s )
{
	const int64_t	chunks = fasta_chunks( text, text_bytes ), blocks = fasta_blocks( chunks );
	if( chunks <= 0 || chunks > 0x7fffffffll )
		return hipErrorInvalidValue;
	const int	lead = int( reinterpret_cast<uintptr_t>( text ) & 3u );
	hipLaunchKernelGGL( rma_fasta_summarise_kernel, dim3( unsigned( chunks ) ), dim3( FD_THREADS ), 0, s,
		words_of( text ), lead, ( long long )( lead + text_bytes ), d_sum );
	hipLaunchKernelGGL( rma_fasta_scan_blocks_kernel, dim3( unsigned( blocks ) ), dim3( FD_THREADS ), 0, s,
		d_sum, ( long long )chunks, d_local, d_block_sum );
	hipLaunchKernelGGL( rma_fasta_scan_top_kernel, dim3( 1 ), dim3( FD_THREADS ), 0, s,
		d_block_sum, ( long long )blocks, d_block_pre, d_totals );
	return hipGetLastError();
}

hipError_t fasta_apply( const uint8_t *text, int64_t text_bytes, const FdSummary *d_local, const FdPrefix *d_block_pre,
	const FdPrefix *d_totals, uint8_t *clean, int64_t *d_gt_off, int64_t *d_def_end, int64_t *d_first, hipStream_t s )
{
	const int64_t	chunks = fasta_chunks( text, text_bytes );
	if( chunks <= 0 || chunks > 0x7fffffffll )
		return hipErrorInvalidValue;
	const int	lead = int( reinterpret_cast<uintptr_t>( text ) & 3u );
	hipLaunchKernelGGL( rma_fasta_apply_kernel, dim3( unsigned( chunks ) ), dim3( FD_THREADS ), 0, s,
		words_of( text ), lead, ( long long )( lead + text_bytes ), d_local, d_block_pre, d_totals, clean,
		reinterpret_cast<long long *>( d_gt_off ), reinterpret_cast<long long *>( d_def_end ), reinterpret_cast<long long *>( d_first ) );
	return hipGetLastError();
}

hipError_t fasta_headers( const uint8_t *text, int64_t text_bytes, const int64_t *d_gt_off, const int64_t *d_def_end,
	const int64_t *d_hdr_off, int64_t n, uint8_t *d_out, hipStream_t s )
{
	if( n <= 0 )
		return hipSuccess;
	hipLaunchKernelGGL( rma_fasta_headers_kernel, dim3( unsigned( ( n + FD_WAVES - 1 ) / FD_WAVES ) ), dim3( FD_THREADS ), 0, s,
		text, ( long long )text_bytes, reinterpret_cast<const long long *>( d_gt_off ), reinterpret_cast<const long long *>( d_def_end ),
		reinterpret_cast<const long long *>( d_hdr_off ), ( long long )n, d_out );
	return hipGetLastError();
}

}	// namespace rma
