// rm_hitct_dev.hip -- see rm_hitct_dev.h
#include <algorithm>
#include <hip/hip_runtime.h>
#include "rm_hitct_dev.h"

namespace rma {

namespace {

constexpr int	HC_BLOCK = 256;
constexpr int	HC_WAVES = HC_BLOCK / 64;

// what a wave keeps of its record in LDS
struct CtWave {
	int32_t	pre[ HC_PRE_ROOM ];		// the letters in front of a field
	int32_t	lo[ 64 ];			// a pass's lines: the first byte of each
	uint8_t	num[ HP_NUM_CAP ], head[ HC_HEAD_CAP ], tail[ HC_TAIL_CAP ];
	uint8_t	line[ 64 ][ HC_LINE_CAP ];
};

// the descriptor's table, for every wave of a workgroup
struct CtTable {
	int16_t	mate[ HA_MAX_COLS ];
	int8_t	kind[ HA_MAX_COLS ];
};

// what hitprint_seg_byte reads, for one record
struct CtSrc {
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

struct CtRec {
	int	code;
	HitPrintIn	in;
	HitCtHead	h;
	float	energy;
};

// what the lanes of one wave have written to LDS is there for all of them behind this
__device__ inline void wave_sync()
{
	__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
}

__device__ inline void table_to_lds( const HitCtBatch &c, CtTable &tab, int t )
{
	for( int i = t; i < HA_MAX_COLS; i += HC_BLOCK ){
		tab.mate[ i ] = c.table.mate[ i ];
		tab.kind[ i ] = c.table.kind[ i ];
	}
}

// Record r of the batch, by its wave: checked; where it is to be written (`accept`) measured by lane 0 and the prefix of
// its field lengths laid into lw.pre.  Of a record only its own words are read, of the tables only the slots of an entry
// that has passed the check, of the score columns only its own.  *src: what its bytes are read from (no letters yet).
__device__ inline CtRec ct_prepare( const HitCtBatch &c, long long r, bool accept, int lane, CtWave &lw, CtSrc *src )
{
	const HitPrintBatch	&b = c.b;
	const int32_t	*w = b.hits + r * b.stride;
	CtRec	rec{ HW_OK, HitPrintIn{ 0, 0, 0, 0 }, HitCtHead{ 0, 0, 0, 0 }, 0.0f };
	int	which;
	rec.code = hitprint_check( w, b.shape, b.n_seq, b.slen, b.text_len[ r ], b.text_width, &which );
	if( rec.code != HW_OK || !accept )
		return rec;
	const int32_t	entry = w[ 0 ];
	const int64_t	*no = b.names.off + 2 * int64_t( entry );
	rec.in = HitPrintIn{ no[ 1 ] - no[ 0 ], no[ 2 ] - no[ 1 ], b.slen[ entry ], b.text_len[ r ] };
	*src = CtSrc{ b.names.bytes + no[ 0 ], b.names.bytes + no[ 1 ], c.text_bytes + ( b.first + r ) * ( long long )b.text_width, lw.num,
		nullptr, nullptr, nullptr, w[ 1 ], rec.in.slen };
	if( lane == 0 ){
		const int	num_len = hitprint_numbers( w, b.shape, rec.in.slen, lw.num, HP_NUM_CAP );
		rec.code = hitct_measure( w, b.shape, rec.in, c.type, num_len, *src, &rec.energy );
	}
	rec.code = __shfl( rec.code, 0 );
	rec.energy = __shfl( rec.energy, 0 );
	if( rec.code != HW_OK )
		return rec;
	// the prefix: lane k has field k and field 64 + k; an inclusive prefix over each pass (no hit line of HC_LINE_SIZE
	// bytes: the sums stay far inside 32 bits)
	const int	n = hitalign_n_cols( b.shape );
	const int32_t	la = lane < n ? hitct_field_len( w, b.shape, lane ) : 0, lb = 64 + lane < n ? hitct_field_len( w, b.shape, 64 + lane ) : 0;
	int32_t	xa = la, xb = lb;
	for( int d = 1; d < 64; d <<= 1 ){
		const int32_t	ua = __shfl_up( xa, d ), ub = __shfl_up( xb, d );
		if( lane >= d ){
			xa += ua;
			xb += ub;
		}
	}
	xb += __shfl( xa, 63 );
	lw.pre[ lane ] = xa - la;
	lw.pre[ 64 + lane ] = xb - lb;
	wave_sync();
	rec.h = hitct_head_of( w, b.shape, rec.in.slen, lw.pre[ n ] );
	return rec;
}

// A wave per record.
__global__ void __launch_bounds__( HC_BLOCK )
rma_hit_ct_size_kernel( HitCtBatch c, int64_t *len_out, unsigned long long *bad )
{
	__shared__ CtWave	s_wave[ HC_WAVES ];
	__shared__ CtTable	s_tab;
	const int	t = threadIdx.x, lane = t & 63, wave = t >> 6;
	table_to_lds( c, s_tab, t );
	__syncthreads();
	const long long	r = blockIdx.x * ( long long )HC_WAVES + wave;
	if( r > c.b.n )
		return;
	if( r == c.b.n ){
		if( lane == 0 )
			len_out[ r ] = 0;
		return;
	}
	CtWave	&lw = s_wave[ wave ];
	CtSrc	src;
	const bool	accept = c.b.accept == nullptr || c.b.accept[ r ] != 0;
	const CtRec	rec = ct_prepare( c, r, accept, lane, lw, &src );
	long long	m = 0;
	if( rec.code != HW_OK ){
		if( lane == 0 )
			atomicMin( bad, ( static_cast<unsigned long long>( c.b.first + r ) << 4 ) | unsigned( rec.code ) );
	}else if( accept ){
		m = hitct_size_part( c.type, s_tab.kind, s_tab.mate, lw.pre, hitalign_n_cols( c.b.shape ), rec.h, rec.energy, rec.in.sid_len, lane, 64 );
		for( int d = 32; d > 0; d >>= 1 )
			m += __shfl_xor( m, d );
	}
	if( lane == 0 )
		len_out[ r ] = m;
}

// the last line k of a pass whose first byte lo[ k ] <= i: the line byte i lies in, the lanes without a line standing
// behind the pass's end
__device__ inline int ct_find_line( const int32_t *lo, int32_t i )
{
	int	a = 0, z = 63;
	while( a < z ){
		const int	mid = ( a + z + 1 ) >> 1;
		if( lo[ mid ] <= i )
			a = mid;
		else
			z = mid - 1;
	}
	return a;
}

// A wave per record.  A record of no bytes (not accepted) has only its offset written.  Nothing outside [ *carry +
// offc[ r ], *carry + offc[ r + 1 ] ) of the output is written for record r -- every store is held to the record's
// bytes as the size kernel counted them --, and nothing outside its entry, its name and its score column is read: the
// record is checked and measured here as it was there.
__global__ void __launch_bounds__( HC_BLOCK )
rma_hit_ct_kernel( HitCtBatch c, const uint8_t *text, const uint8_t *table, int codes, const int64_t *offc, const int64_t *carry, uint8_t *out,
	int64_t *off_out, int last )
{
	__shared__ uint8_t	let[ 256 ], cmp[ 256 ];		// byte -> its letter, the complement of its letter
	__shared__ CtWave	s_wave[ HC_WAVES ];
	__shared__ CtTable	s_tab;
	const int	t = threadIdx.x, lane = t & 63, wave = t >> 6;
	{
		const unsigned char	v = table[ t ];
		const unsigned char	l = codes ? hitwin_code_letter( v ) : v;
		let[ t ] = l;
		cmp[ t ] = hitwin_wc_cmp( l );
	}
	table_to_lds( c, s_tab, t );
	__syncthreads();
	const HitPrintBatch	&b = c.b;
	CtWave	&lw = s_wave[ wave ];
	const int	n = hitalign_n_cols( b.shape );
	const int64_t	before = *carry;
	for( long long r = blockIdx.x * ( long long )HC_WAVES + wave; r < b.n; r += gridDim.x * ( long long )HC_WAVES ){
		const int64_t	o = offc[ r ], m = offc[ r + 1 ] - o;
		if( lane == 0 ){
			off_out[ r ] = before + o;
			if( last && r == b.n - 1 )
				off_out[ b.n ] = before + offc[ b.n ];
		}
		if( m <= 0 )
			continue;
		CtSrc	src;
		const CtRec	rec = ct_prepare( c, r, true, lane, lw, &src );
		if( rec.code != HW_OK )
			continue;
		const int32_t	*w = b.hits + r * b.stride;
		src.entry_p = text + b.start[ w[ 0 ] ];
		src.let = let;
		src.cmp = cmp;
		// the header line: its two halves, once
		int	hl = 0, tl = 0;
		if( lane == 0 ){
			hl = hitct_head( c.type, rec.h, rec.energy, lw.head, HC_HEAD_CAP );
			tl = hitct_tail( c.type, rec.h, lw.tail, HC_TAIL_CAP );
		}
		hl = __shfl( hl, 0 );
		tl = __shfl( tl, 0 );
		wave_sync();
		uint8_t	*dst = out + before + o;
		int64_t	base = hl + rec.in.sid_len + tl;
		for( int64_t j = lane; j < base && j < m; j += 64 )
			dst[ j ] = j < hl ? lw.head[ j ] : j < hl + rec.in.sid_len ? src.sid( j - hl ) : lw.tail[ j - hl - rec.in.sid_len ];
		// the bases' lines, 64 at a time
		for( int32_t p0 = 0; p0 < rec.h.nb; p0 += 64 ){
			const int32_t	bn = p0 + lane + 1;
			int32_t	len = 0;
			if( bn <= rec.h.nb ){
				int	f;
				int32_t	k, pn;
				const int32_t	hn = hitct_base( s_tab.kind, s_tab.mate, lw.pre, n, rec.h, bn, &f, &k, &pn );
				const uint8_t	letter = src.letter( w[ hitstruct_word( b.shape, hitalign_col_elem( b.shape, f ) ) ] + k );
				len = hitct_line( c.type, bn, rec.h.nb, letter, pn, hn, lw.line[ lane ], HC_LINE_CAP );
			}
			int32_t	x = len;
			for( int d = 1; d < 64; d <<= 1 ){
				const int32_t	u = __shfl_up( x, d );
				if( lane >= d )
					x += u;
			}
			lw.lo[ lane ] = x - len;
			const int32_t	total = __shfl( x, 63 );
			wave_sync();
			for( int32_t i = lane; i < total && base + i < m; i += 64 ){
				const int	ln = ct_find_line( lw.lo, i );
				dst[ base + i ] = lw.line[ ln ][ i - lw.lo[ ln ] ];
			}
			base += total;
			wave_sync();
		}
	}
}

}	// namespace

hipError_t hit_ct_sizes( const HitCtBatch &c, int64_t *d_len, unsigned long long *d_bad, hipStream_t s )
{
	if( c.b.n < 0 )
		return hipErrorInvalidValue;
	hipLaunchKernelGGL( rma_hit_ct_size_kernel, dim3( unsigned( ( c.b.n + 1 + HC_WAVES - 1 ) / HC_WAVES ) ), dim3( HC_BLOCK ), 0, s, c, d_len, d_bad );
	return hipGetLastError();
}

hipError_t hit_ct_fill( const HitCtBatch &c, const uint8_t *text, const uint8_t *table, int codes, const int64_t *d_offc, const int64_t *d_carry,
	uint8_t *d_out, int64_t *d_off, bool last, hipStream_t s )
{
	if( c.b.n <= 0 )
		return c.b.n < 0 ? hipErrorInvalidValue : hipSuccess;
	const int64_t	blocks = std::min<int64_t>( ( c.b.n + HC_WAVES - 1 ) / HC_WAVES, 4096 );
	hipLaunchKernelGGL( rma_hit_ct_kernel, dim3( unsigned( blocks ) ), dim3( HC_BLOCK ), 0, s, c, text, table, codes, d_offc, d_carry, d_out, d_off,
		last ? 1 : 0 );
	return hipGetLastError();
}

}	// namespace rma
