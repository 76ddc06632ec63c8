// passa_check.cpp -- TEST INFRASTRUCTURE.
//
// Two things the search kernel that walks nothing (rm_scan_kernel.h, RMK_LEAN_FLUSH / RMK_LEAN_CONCAT_FLUSH) does behind
// its pre-filter, on the CPU, with the rules as rm_scan_core.h states them for host and device:
//
//   * the end window of the look-ahead chain (rmd_chain_t, rm_dev_program.cpp) loses no candidate: for every record the
//     oracle finds, the vector E that the kernel ANDs onto the end positions of the first search element's group has its bit
//     at the record's end position; and where E is decided it says what the rule says, tested base by base;
//   * pass A' on quads of lanes (rmd_passa_quads) gives every item the (keep, hm0, hm1) of the sequential loop it replaces,
//     which is copied below as the reference, with the masks wanted and not wanted.
//
//   passa_check SEQS [rnamotif options] -descr file.descr
// SEQS: a file of entries, one per line.  Every entry is scanned by the oracle on both strands; its vectors -- where each
// base stands, the pair rows, the stem-loops' cores, E -- are built as the kernel builds them, for the entry as one tile and
// cut into tiles of 96 and 512 start positions, each array in a heap block of exactly its size (a build with
// -fsanitize=address sees a read past either end).  Items: the start positions of a tile (every third in long entries)
// with every span the first element's group may have.
// Prints "end_window on=.. d_lo=.. d_hi=.. slot=.. chain_on=.. n=..", "tests tail=.. head=.. head_next=.. lengths=..
// pre=..", "records N checked M lost K wrong W set S of P" and "items N differ D kept K masked M"; exit status 1 when a
// candidate is lost, a decided bit is wrong or an item differs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "rm_cli.h"
#include "rm_dev_program.h"
#include "rm_scan_core.h"
extern "C" {
#include "rm_oracle.h"
}

struct Tile {
	int	p_lo, p_to, vec_words;
	std::vector<uint8_t>	bytes;			// the byte per base: 0 .. 3, 4 for a letter that is not acgt, 7 outside the entry
	std::vector<unsigned long long>	pb, tv, E;	// five pair rows; the chain's ten vectors (0 .. 4: where each base stands, 7 .. 9: cores)
};

static int code_of( char c )
{
	switch( c ){
	case 'a': case 'A': return 0;
	case 'c': case 'C': return 1;
	case 'g': case 'G': return 2;
	case 't': case 'T': case 'u': case 'U': return 3;
	}
	return 4;
}

// the kernel's pairs(): the bases at x .. x+63 pair with the ones d further on; outside the vectors: undecided, kept
static unsigned long long pairs( const Tile &t, int nb, int x, int d )
{
	const int	vec_bits = t.vec_words * 64, W = t.vec_words;
	const bool	in5 = x >= 0 && x + 96 <= vec_bits, in3 = x + d >= 0 && x + d + 96 <= vec_bits;
	unsigned long long	m = 0;
	for( int b = 0; b < nb; b++ )
		m |= ( in5 ? rmd_bits64( t.tv.data() + b * W, x ) : ~0ull ) & ( in3 ? rmd_bits64( t.pb.data() + b * W, x + d ) : ~0ull );
	return m;
}

// what the kernel holds of the positions [ p_lo, p_to ) of an entry: bit q - p_lo + 64 of a vector is position q
static Tile make_tile( const std::vector<int> &codes, int p_lo, int p_to, int n_bytes, unsigned mat2, const rmd_chain_t &ch, bool e_on )
{
	Tile	t;
	t.p_lo = p_lo;
	t.p_to = p_to;
	t.vec_words = ( p_to - p_lo + 64 + 63 ) / 64 + 1;
	const int	W = t.vec_words, vec_bits = W * 64, nb = ( ( mat2 >> 20 ) & 31u ) || ( mat2 & 0x0108421u << 4 ) ? 5 : 4;
	t.bytes.assign( n_bytes, 7 );
	t.pb.assign( 5 * W, 0ull );
	t.tv.assign( 10 * W, 0ull );
	for( int q = std::max( p_lo, 0 ); q < p_to; q++ ){
		const int	bit = q - p_lo + 64, c = codes[ q ];
		t.bytes[ q - p_lo ] = uint8_t( c );
		t.tv[ c * W + ( bit >> 6 ) ] |= 1ull << ( bit & 63 );
		for( int b5 = 0; b5 < 5; b5++ )
			if( ( mat2 >> ( b5 * 5 + c ) ) & 1u )
				t.pb[ b5 * W + ( bit >> 6 ) ] |= 1ull << ( bit & 63 );
	}
	for( int k = ch.n - 1; k >= 0; k-- ){
		const rmd_chain_sib_t	&sb = ch.sib[ k ];
		if( !sb.leaf )
			continue;
		unsigned long long	*core = t.tv.data() + ( 7 + ( sb.core_slot >= 0 ? sb.core_slot : 2 ) ) * W;
		for( int wi = 0; wi < W; wi++ ){
			unsigned long long	f = 0;
			for( int L = sb.lmin; L <= sb.lmax; L++ ){
				unsigned long long	w1 = ~0ull;
				for( int j = 0; j < sb.hmin; j++ )
					w1 &= pairs( t, nb, wi * 64 + j, 2 * sb.hmin + L - 1 - 2 * j );
				f |= w1;
			}
			core[ wi ] = f;
		}
	}
	if( e_on ){
		const rmd_chain_sib_t	&en = ch.sib[ ch.n ];
		t.E.assign( W, 0ull );
		for( int wi = 0; wi < W; wi++ )
			t.E[ wi ] = rmd_or_window( t.tv.data() + ( 7 + en.core_slot ) * W, wi * 64 - en.len_hi, 0, en.len_hi - en.len_lo, vec_bits );
	}
	return t;
}

// the end window's rule itself: some d in the window has the stem-loop's innermost hmin pairs, for one of its loop lengths, d before e
static bool direct( const std::vector<int> &codes, unsigned mat2, const rmd_chain_sib_t &leaf, const rmd_chain_sib_t &en, int e )
{
	const int	slen = int( codes.size() );
	for( int d = en.len_lo; d <= en.len_hi; d++ )
		for( int L = leaf.lmin; L <= leaf.lmax; L++ ){
			const int	c = e - d;
			if( c < 0 || c + 2 * leaf.hmin + L > slen )
				continue;
			bool	ok = true;
			for( int j = 0; j < leaf.hmin && ok; j++ )
				ok = ( mat2 >> ( codes[ c + j ] * 5 + codes[ c + 2 * leaf.hmin + L - 1 - j ] ) ) & 1u;
			if( ok )
				return true;
		}
	return false;
}

// REFERENCE: pass A' of the search kernel as it stood before the quads, one lane an item, the outer lengths one after the
// other and the tail before the head (rm_scan_kernel.h at 8268a15, the body of `if( ( tail_from_rows || head_from_rows ) && r != 0xffff )`)
static void sequential( const rmd_passa_t &A, const rmd_elem_t &e0, int szero, int span, bool want_masks, bool *keep_out, unsigned *hm )
{
	const rmd_program_t	*P = A.P;
	bool	keep = false;
	hm[ 0 ] = hm[ 1 ] = ~0u;
	if( want_masks )
		hm[ 0 ] = hm[ 1 ] = 0;
	for( int hl = e0.minlen; hl <= e0.maxlen && ( !keep || want_masks ); hl++ ){
		const int	ilen = span - 2 * hl;
		if( ilen < e0.minilen )
			break;
		if( ilen > e0.maxilen )
			continue;
		unsigned	ends_left = ~0u;
		bool	ok = true, t;
		const TailAccel	ac{ P, A.pb, A.tile, A.pb_words, A.p_lo, A.vec_bits, 0 };
		if( A.tail_from_rows && ac.tail( e0, szero, hl, span - 1 - hl, &t ) )
			ok = t;
		if( ok && A.head_from_rows ){
			const rmd_elem_t	&H = P->elems[ P->searches[ e0.head_s ] ];
			const int	lim = ( H.ends & RMA_5PAIRED ) ? H.mplim : ( H.mplim > 1 ? H.mplim : 1 );
			const int	b = szero + span - 1 - hl;		// last position of the interior
			ok = false;
			for( int pre = e0.head_pre_min; pre <= e0.head_pre_max && !ok; pre++ ){
				const int	s5 = szero + hl + pre;
				const int	top = rmd_imin( s5 + H.maxglen - 1, b ), bot = s5 + H.minglen - 1;
				if( top < bot )
					continue;
				const int	w0 = top - 63, q_hi = w0 - A.p_lo + 64;
				if( top - bot >= 64 || q_hi - H.minlen < 0 || q_hi + 96 > A.vec_bits )
					ok = true;
				else{
					unsigned long long	Wd = rmd_rows_win( A.pb, A.pb_words, A.tile, A.p_lo, H.minlen, lim, ( H.ends & RMA_5PAIRED ) != 0, s5, w0, bot );
					if( !A.all_ends ){
						const int	e_hi = rmd_imin( top, b - H.rem_min ) - w0, e_lo = ( H.rem_max >= 0 ? rmd_imax( bot, b - H.rem_max ) : bot ) - w0;
						if( e_hi < 63 )
							Wd &= e_hi < 0 ? 0ull : ( 2ull << e_hi ) - 1;
						if( e_lo > 0 )
							Wd &= e_lo > 63 ? 0ull : ~0ull << e_lo;
					}
					if( Wd && A.head_next ){
						const rmd_chain_t	&C = P->chain;
						const int	x = w0 - A.p_lo + 64, g_lo = C.hn_glo + 1, g_hi = C.hn_ghi + 1 + C.hn_tmax;
						const bool	all = g_hi < g_lo || ( x + g_lo >= 0 && x + g_hi + 96 <= A.vec_bits );
						if( all )
							Wd &= rmd_or_window( A.tv + ( 7 + C.hn_slot ) * A.pb_words, x, g_lo, g_hi, A.vec_bits );
						if( all && top - bot < 32 )
							ends_left = unsigned( Wd >> ( bot - w0 ) );
					}
					ok = Wd != 0;
				}
			}
		}
		if( ok && hl - e0.minlen < 2 )
			hm[ hl - e0.minlen ] = want_masks ? ends_left : ~0u;
		if( ok && hl - e0.minlen >= 2 )
			hm[ 0 ] = hm[ 1 ] = ~0u, keep = true;
		keep = keep || ok;
	}
	*keep_out = keep;
}

int main( int argc, char **argv )
{
	if( argc < 3 ){
		fprintf( stderr, "usage: passa_check SEQS [rnamotif options] -descr file.descr\n" );
		return 2;
	}
	std::vector<char *>	args{ argv[ 0 ] };
	for( int i = 2; i < argc; i++ )
		args.push_back( argv[ i ] );
	rma::Prepared	pr = rma::prepare( rma::parse_args( int( args.size() ), args.data() ) );
	std::vector<rmd_program_t>	dpv( 1 );
	rmd_program_t	&dp = dpv[ 0 ];
	char	err[ 512 ];
	if( rmd_build( pr.prog.get(), &dp, err, sizeof( err ) ) ){
		fprintf( stderr, "rmd_build: %s\n", err );
		return 2;
	}
	const rmd_chain_t	&ch = dp.chain;
	const rmd_elem_t	&e0 = dp.elems[ dp.searches[ 0 ] ];
	if( !ch.on || e0.type != RMA_T_H5 || e0.rows != 0 ){
		fprintf( stderr, "no look-ahead chain: not a descriptor for the kernel that walks nothing\n" );
		return 2;
	}
	const bool	on = ch.n < RMD_MAX_CHAIN && ch.sib[ ch.n ].end_on;
	const rmd_chain_sib_t	en = ch.sib[ on ? ch.n : 0 ], leaf = ch.sib[ ch.n - 1 ];
	printf( "end_window on=%d d_lo=%d d_hi=%d slot=%d chain_on=%d n=%d\n", int( on ), on ? int( en.len_lo ) : 0, on ? int( en.len_hi ) : 0,
		on ? int( en.core_slot ) : -1, int( ch.on ), int( ch.n ) );
	if( on && ( !leaf.leaf || leaf.core_slot != en.core_slot ) ){
		fprintf( stderr, "the end window does not name the chain's last stem-loop\n" );
		return 1;
	}
	const unsigned	mat2 = dp.pairsets[ e0.pairset ].mat2;
	// which tests pass A' runs: the kernel's own conditions (rma_search_kernel: tail_from_rows, head_from_rows, head_next)
	bool	tail_from_rows = false;
	if( e0.tail_s >= 0 ){
		const rmd_elem_t	&te = dp.elems[ dp.searches[ e0.tail_s ] ];
		bool	sym = true;
		for( int x = 0; x < 5; x++ )
			for( int y = 0; y < 5; y++ )
				sym = sym && ( ( ( mat2 >> ( x * 5 + y ) ) ^ ( mat2 >> ( y * 5 + x ) ) ) & 1 ) == 0;
		tail_from_rows = sym && te.pairset == e0.pairset && te.mplim == 0 && !te.pfrac && te.minlen >= 1 &&
			( te.ends & RMA_5PAIRED ) && ( te.ends & RMA_3PAIRED ) && te.maxglen != RMA_UNBOUNDED;
	}
	const bool	head_from_rows = e0.head_s >= 0 && dp.elems[ dp.searches[ e0.head_s >= 0 ? e0.head_s : 0 ] ].rows == 0;
	printf( "tests tail=%d head=%d head_next=%d lengths=%d pre=%d\n", int( tail_from_rows ), int( head_from_rows ), int( ch.hn_on ),
		e0.maxlen - e0.minlen + 1, head_from_rows ? e0.head_pre_max - e0.head_pre_min + 1 : 0 );
	const int	d3 = e0.mates[ 0 ], w = dp.w_winsize, lm = dp.lmargin, rm = dp.rmargin;
	long long	n_rec = 0, n_checked = 0, n_lost = 0, n_wrong = 0, n_set = 0, n_pos = 0;
	long long	n_items = 0, n_differ = 0, n_kept = 0, n_masked = 0;
	std::ifstream	in( argv[ 1 ] );
	std::string	line;
	static const int	tiles[] = { 0, 96, 512 };	// (0: the entry as one tile)
	for( int seq = 0; std::getline( in, line ); seq++ ){
		const int	slen = int( line.size() );
		for( int comp = 0; comp < ( pr.prog->chk_both_strs ? 2 : 1 ); comp++ ){
			std::vector<char>	buf( line.begin(), line.end() );
			buf.push_back( '\0' );
			if( comp )
				rmo_revcomp( buf.data(), slen );
			rmo_hits_t	oh;
			rmo_hits_init( &oh, pr.prog.get() );
			rmo_set_efn2data( pr.efn2.get() );
			if( rmo_scan( pr.prog.get(), pr.efn.get(), seq, buf.data(), slen, comp, &oh ) ){
				fprintf( stderr, "rmo_scan failed\n" );
				return 2;
			}
			n_rec += oh.n;
			std::vector<int>	codes( slen );
			for( int q = 0; q < slen; q++ )
				codes[ q ] = code_of( buf[ q ] );
			for( int T : tiles ){
				const int	tt = T ? T : std::max( slen, 1 );
				for( int z0 = 0; z0 < slen; z0 += tt ){
					int	p_lo = z0 - lm;
					p_lo -= ( ( p_lo % 32 ) + 32 ) % 32;
					// (the bytes reach as far as the kernel's tile: tile_t + w - 1 + margins; the entry may end before)
					const int	p_end = z0 + tt + w - 1 + rm, p_to = std::min( slen, p_end );
					const Tile	t = make_tile( codes, p_lo, p_to, p_end - p_lo + 32, mat2, ch, on );
					const int	vec_bits = t.vec_words * 64;
					if( on ){
						// decided bits say what the rule says
						for( int e = std::max( p_lo, 0 ); e + 64 <= p_to; e++ ){		// (cores near the vector's end are undecided themselves)
							const int	x = e - p_lo + 64, wx = ( x >> 6 ) * 64;
							// (a word of E is decided when its window stayed inside the vector: rmd_or_window)
							if( wx - en.len_hi < 0 || wx - en.len_lo + 96 > vec_bits || x + 96 > vec_bits )
								continue;
							// (the tile holds no bases below p_lo: a core there belongs to no item of this tile, whose start positions lie above)
							if( e - en.len_hi < p_lo )
								continue;
							const bool	bit = ( rmd_bits64( t.E.data(), x ) & 1ull ) != 0;
							n_pos++;
							n_set += bit;
							if( bit != direct( codes, mat2, leaf, en, e ) && n_wrong++ < 10 )
								fprintf( stderr, "seq %d comp %d tile %d z0 %d: E at %d is %d, the rule says otherwise\n", seq, comp, T, z0, e, int( bit ) );
						}
						// no record loses its end position
						for( long long h = 0; h < oh.n; h++ ){
							const int32_t	*r = oh.data + h * oh.stride;
							if( r[ 2 ] < z0 || r[ 2 ] >= z0 + tt )
								continue;
							const int	e = r[ RMA_HIT_HDR + 4 * d3 ] + r[ RMA_HIT_HDR + 4 * d3 + 1 ] - 1;
							n_checked++;
							if( !( rmd_peek( t.E.data(), e - p_lo + 64, vec_bits ) & 1ull ) && n_lost++ < 10 )
								fprintf( stderr, "seq %d comp %d tile %d z0 %d: the record at %d that ends at %d has no bit in E\n", seq, comp, T, z0, r[ 2 ], e );
							if( !direct( codes, mat2, leaf, en, e ) && n_lost++ < 10 )
								fprintf( stderr, "seq %d comp %d: the record at %d that ends at %d fails the rule\n", seq, comp, r[ 2 ], e );
						}
					}
					if( tail_from_rows || head_from_rows ){
						// the quads against the sequential loop: every item the pre-filter could queue in this tile
						const int	step = slen > 1000 ? 3 : 1;
						for( int hn = 0; hn < ( ch.hn_on ? 2 : 1 ); hn++ ){
							const rmd_passa_t	A{ &dp, t.pb.data(), t.tv.data(), t.bytes.data(), t.vec_words, p_lo, vec_bits, tail_from_rows, head_from_rows,
								hn != 0, false };
							const bool	want_masks = A.head_next && e0.head_pre_min == e0.head_pre_max;
							for( int szero = z0; szero < std::min( z0 + tt, slen ); szero += step )
								for( int span = e0.minglen; span <= std::min( e0.maxglen, slen - szero ); span++ ){
									bool	k_ref, k_got;
									unsigned	h_ref[ 2 ], h_got[ 2 ];
									sequential( A, e0, szero, span, want_masks, &k_ref, h_ref );
									rmd_passa_quads( A, e0, szero, span, want_masks, &k_got, &h_got[ 0 ], &h_got[ 1 ] );
									n_items++;
									n_kept += k_ref;
									n_masked += k_ref && ( ( h_ref[ 0 ] != 0 && h_ref[ 0 ] != ~0u ) || ( h_ref[ 1 ] != 0 && h_ref[ 1 ] != ~0u ) );
									if( ( k_ref != k_got || h_ref[ 0 ] != h_got[ 0 ] || h_ref[ 1 ] != h_got[ 1 ] ) && n_differ++ < 10 )
										fprintf( stderr, "seq %d comp %d tile %d z0 %d item %d+%d masks %d: (%d %08x %08x), the loop (%d %08x %08x)\n", seq, comp, T, z0,
											szero, span, int( want_masks ), int( k_got ), h_got[ 0 ], h_got[ 1 ], int( k_ref ), h_ref[ 0 ], h_ref[ 1 ] );
								}
						}
					}
				}
			}
			rmo_hits_free( &oh );
		}
	}
	printf( "records %lld checked %lld lost %lld wrong %lld set %lld of %lld\n", n_rec, n_checked, n_lost, n_wrong, n_set, n_pos );
	printf( "items %lld differ %lld kept %lld masked %lld\n", n_items, n_differ, n_kept, n_masked );
	return n_lost || n_wrong || n_differ ? 1 : 0;
}
