// efn_window_check.cpp -- TEST INFRASTRUCTURE.
//
// The energy kernel's way to the bases of a call, compiled for the CPU over a database packed with the project's
// packer (rm_pack.cpp), the packed words in heap blocks of exactly their size:
//   (i)  rmw_window_codes() (rm_seq_window.h) against the rule of the kernels' db_code(), restated here base by base:
//        every start, every length 1..96, both strands, on entries of the test's own (shorter than a word, letters
//        under the mask at every place of a window) and on the file's first and last entries;
//   (ii) rme_cand_t::fill_cache() for every candidate the oracle finds in the file, every efn()/efn2() site: cbc[]/cbp[]
//        against the uncached bc()/bp(), and the site's energy cached against uncached against the oracle's -- with
//        a Seq that has window(), with one that has only code(), and with the elements' facts laid out as the kernel
//        has them.
//
//   efn_window_check [rnamotif options] -descr file.descr db.fastn
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rm_cli.h"
#include "rm_pack.h"
#include "rm_oracle.h"
#define RMD_FN static inline
#define RMD_FN_MEMBER inline
#include "rm_efn_core.h"
#include "rm_efn2_core.h"
#include "rm_efndata.h"

// the packed database as the kernels see it: blocks of exactly the words' size
struct Words {
	uint32_t	*codes = nullptr, *amask = nullptr;
	size_t	n_codes = 0, n_amask = 0;
};

// db_code() / db_strand_code() of rm_scan_kernel.h
static int ref_code( const Words &W, int64_t off, int slen, int comp, int p )
{
	const int64_t	base = off + ( comp ? slen - 1 - p : p );
	if( size_t( base >> 5 ) >= W.n_amask || size_t( base >> 4 ) >= W.n_codes ){
		fprintf( stderr, "ref_code: base %lld outside the pack\n", ( long long )base );
		exit( 2 );
	}
	if( ( W.amask[ base >> 5 ] >> ( base & 31 ) ) & 1 )
		return RMA_BC_N;
	const int	c = ( W.codes[ base >> 4 ] >> ( 2 * ( base & 15 ) ) ) & 3;
	return comp ? 3 - c : c;
}

struct CodeSeq {			// code() only: fill_cache() goes base by base
	const Words	*W;
	int64_t	off;
	int	slen, comp;
	int	code( int p ) const { return ref_code( *W, off, slen, comp, p ); }
};
struct BulkSeq : CodeSeq {		// ... and window(), as the kernel's DevSeq
	void	window( int p, int n, uint8_t *out ) const { rmw_window_codes( W->codes, W->amask, off, slen, comp, p, n, out ); }
};
static_assert( !rme_has_window<CodeSeq>::value && rme_has_window<BulkSeq>::value, "the two kinds of Seq" );

static long long	bad = 0;
#define FAIL( ... )	do{ if( bad++ < 20 ){ fprintf( stderr, __VA_ARGS__ ); fputc( '\n', stderr ); } }while( 0 )

struct WinStats { long long windows = 0, n_first = 0, n_last = 0, n_inner = 0, exact = 0; };

// one window, against the rule; exact: once more over copies of just the words that hold a base of it
static void check_window( const Words &W, int64_t off, int slen, int comp, int p, int n, bool exact, WinStats &st )
{
	uint8_t	*out = static_cast<uint8_t *>( malloc( n ) );
	rmw_window_codes( W.codes, W.amask, off, slen, comp, p, n, out );
	for( int i = 0; i < n; i++ ){
		const int	want = ref_code( W, off, slen, comp, p + i );
		if( out[ i ] != want )
			FAIL( "window off %lld slen %d comp %d p %d n %d: base %d is %d, the rule gives %d", ( long long )off, slen, comp, p, n, i, out[ i ], want );
		if( want == RMA_BC_N ){
			if( i == 0 ) st.n_first++;
			if( i == n - 1 ) st.n_last++;
			if( i > 0 && i < n - 1 ) st.n_inner++;
		}
	}
	st.windows++;
	if( exact ){
		const int64_t	f0 = off + ( comp ? slen - p - n : p ), f1 = f0 + n - 1;
		const int64_t	a0 = f0 >> 5, a1 = f1 >> 5, c1 = f1 >> 4;
		Words	X;
		X.n_amask = size_t( a1 - a0 + 1 );
		X.n_codes = size_t( c1 - 2 * a0 + 1 );
		X.amask = static_cast<uint32_t *>( malloc( X.n_amask * 4 ) );
		X.codes = static_cast<uint32_t *>( malloc( X.n_codes * 4 ) );
		memcpy( X.amask, W.amask + a0, X.n_amask * 4 );
		memcpy( X.codes, W.codes + 2 * a0, X.n_codes * 4 );
		uint8_t	*out2 = static_cast<uint8_t *>( malloc( n ) );
		rmw_window_codes( X.codes, X.amask, off - 32 * a0, slen, comp, p, n, out2 );
		if( memcmp( out, out2, n ) )
			FAIL( "window off %lld slen %d comp %d p %d n %d: differs over copies of its own words", ( long long )off, slen, comp, p, n );
		free( out2 );
		free( X.amask );
		free( X.codes );
		st.exact++;
	}
	free( out );
}

// every window of an entry that begins in its first 32 positions or ends in its last 32, n = 1 .. 96 (a short entry: all)
static void check_entry( const Words &W, int64_t off, int slen, bool exact, WinStats &st )
{
	for( int comp = 0; comp < 2; comp++ )
		for( int n = 1; n <= RMW_MAX && n <= slen; n++ ){
			const int	last = slen - n;	// last start
			for( int p = 0; p <= last; p++ ){
				if( p >= 32 && p < last - 31 ){
					p = last - 32;
					continue;
				}
				check_window( W, off, slen, comp, p, n, exact, st );
			}
		}
}

static std::string synthetic( unsigned seed, int len, const std::vector<int> &ns )
{
	std::string	s( size_t( len ), 'a' );
	for( int i = 0; i < len; i++ ){
		seed = seed * 1664525u + 1013904223u;
		s[ i ] = "acgt"[ ( seed >> 24 ) & 3 ];
	}
	for( int q : ns )
		if( q >= 0 && q < len )
			s[ q ] = 'n';
	return s;
}

struct SiteStats { long long cands = 0, sites = 0, cached = 0, longer = 0, rejected = 0; };

template< class Seq, int BIG >
static void check_sites( const rmd_program_t &dp, const rma::Prepared &pr, const rme_tables_t &T16, const std::vector<rme_el_t> &facts,
	const Seq &sq, const int32_t *w, const int32_t *oracle_e, const char *what, SiteStats *st )
{
	for( int k = 0; k < dp.n_efn; k++ ){
		const bool	is2 = dp.efn_sites[ k ].kind == RMA_EFN_KIND_EFN2;
		if( is2 ? !pr.efn2 : !pr.efn )
			continue;
		rme_cand_t<Seq>	c;
		c.P = &dp;
		c.w = w;
		c.sq = &sq;
		const int	ok = c.setup( dp.efn_sites[ k ] );
		if( st ){
			st->sites++;
			if( !ok ) st->rejected++;
			else if( c.len <= RMW_MAX ) st->cached++;
			else st->longer++;
		}
		if( ok && c.len <= RMW_MAX ){
			// blocks of exactly the call's size: fill_cache() writes [ 0, len ) of each and nothing else
			int16_t	*bp = static_cast<int16_t *>( malloc( size_t( c.len ) * sizeof( int16_t ) ) );
			uint8_t	*bc = static_cast<uint8_t *>( malloc( size_t( c.len ) ) );
			rme_cand_t<Seq>	cc = c;
			cc.fill_cache( bp, bc );
			for( int i = -1; i <= c.len; i++ ){
				if( cc.bc( i ) != c.bc( i ) )
					FAIL( "%s: site %d base %d of %d: cached code %d, uncached %d", what, k, i, c.len, cc.bc( i ), c.bc( i ) );
				if( cc.bp( i ) != c.bp( i ) )
					FAIL( "%s: site %d base %d of %d: cached partner %d, uncached %d", what, k, i, c.len, cc.bp( i ), c.bp( i ) );
			}
			free( bp );
			free( bc );
		}
		int16_t	bpbuf[ RMW_MAX + 2 ];
		uint8_t	bcbuf[ RMW_MAX + 4 ];
		int	plain, cached, kern;
		if( is2 ){
			plain = rme2_site_energy<Seq, BIG>( &dp, pr.efn2.get(), &sq, w, k );
			cached = rme2_site_energy<Seq, BIG>( &dp, pr.efn2.get(), &sq, w, k, bpbuf, bcbuf, RMW_MAX );
			kern = rme2_site_energy<Seq, BIG, true>( &dp, pr.efn2.get(), &sq, w, k, bpbuf, bcbuf, RMW_MAX, facts.data() );
		}else{
			plain = rme_site_energy<Seq, BIG>( &dp, &T16, &sq, w, k );
			cached = rme_site_energy<Seq, BIG>( &dp, &T16, &sq, w, k, bpbuf, bcbuf, RMW_MAX );
			kern = rme_site_energy<Seq, BIG, true>( &dp, &T16, &sq, w, k, bpbuf, bcbuf, RMW_MAX, facts.data() );
		}
		if( plain != oracle_e[ k ] || cached != plain || kern != plain )
			FAIL( "%s: site %d: oracle %d, uncached %d, cached %d, cached with the elements' facts %d", what, k, oracle_e[ k ], plain, cached, kern );
	}
}

int main( int argc, char **argv )
{
	try{
		rma::Args	args = rma::parse_args( argc, argv );
		rma::Prepared	pr = rma::prepare( args );
		rmd_program_t	dp;
		char	err[ 512 ];
		if( rmd_build( pr.prog.get(), &dp, err, sizeof( err ) ) ){
			fprintf( stderr, "rmd_build: %s\n", err );
			return 2;
		}
		// the pack: an entry of the test's own, the file's entries, two more of the test's own
		std::vector<rma::SeqRecord>	recs;
		for( const std::string &fn : args.dbfnames ){
			FILE	*fp = fopen( fn.c_str(), "r" );
			if( !fp ){ perror( fn.c_str() ); return 2; }
			rma::FastaReader	rd( fp );
			rma::SeqRecord	rec;
			while( rd.next( rec ) )
				recs.push_back( rec );
			fclose( fp );
		}
		if( recs.empty() ){
			fprintf( stderr, "no entries\n" );
			return 2;
		}
		rma::PackFile	pf;
		rma::SeqRecord	own;
		own.sid = "own0";
		own.seq = synthetic( 1, 19, { 0, 7, 18 } );				// shorter than a word of the mask
		pf.add( own );
		for( const rma::SeqRecord &r : recs )
			pf.add( r );
		own.sid = "own1";
		own.seq = synthetic( 2, 31, { 30 } );
		pf.add( own );
		own.sid = "own2";
		own.seq = synthetic( 3, 203, { 0, 5, 15, 16, 31, 32, 47, 63, 64, 95, 96, 100, 127, 128, 170, 201, 202 } );	// the pack's last entry
		pf.add( own );
		Words	W;
		W.n_codes = pf.codes.size();
		W.n_amask = pf.amask.size();
		W.codes = static_cast<uint32_t *>( malloc( W.n_codes * 4 ) );
		W.amask = static_cast<uint32_t *>( malloc( W.n_amask * 4 ) );
		memcpy( W.codes, pf.codes.data(), W.n_codes * 4 );
		memcpy( W.amask, pf.amask.data(), W.n_amask * 4 );
		const int	n_ent = pf.count();

		// (i)
		WinStats	ws;
		for( int e : { 0, n_ent - 2, n_ent - 1 } )
			check_entry( W, pf.base_off[ e ], pf.slen[ e ], true, ws );
		check_entry( W, pf.base_off[ 1 ], pf.slen[ 1 ], false, ws );			// the file's first entry
		check_entry( W, pf.base_off[ n_ent - 3 ], pf.slen[ n_ent - 3 ], false, ws );	// ... and its last
		if( ws.n_first == 0 || ws.n_last == 0 || ws.n_inner == 0 ){
			fprintf( stderr, "no window with a letter under the mask at its first / last / an inner place\n" );
			return 2;
		}
		printf( "windows: %lld checked (%lld over copies of their own words), letters under the mask: %lld first, %lld last, %lld inner\n",
			ws.windows, ws.exact, ws.n_first, ws.n_last, ws.n_inner );

		// (ii)
		std::vector<int16_t>	t16;
		std::vector<int32_t>	tlkey;
		if( pr.efn )
			rma::efn_tables16( pr.efn.get(), t16, tlkey );
		const rme_tables_t	T16{ t16.data(), tlkey.data(), pr.efn ? pr.efn->loginc : nullptr };
		std::vector<rme_el_t>	facts;
		for( int d = 0; d < dp.n_elems; d++ )
			facts.push_back( rme_el_of( &dp, d ) );
		const int	stride = dp.hit_stride, n_cmp = rma_hit_efn_off( pr.prog.get() );
		SiteStats	ss;
		for( size_t r = 0; r < recs.size(); r++ ){
			std::vector<char>	buf( recs[ r ].seq.begin(), recs[ r ].seq.end() );
			buf.push_back( 0 );
			const int	slen = int( recs[ r ].seq.size() ), ent = int( r ) + 1;
			for( int comp = 0; comp < ( pr.prog->chk_both_strs ? 2 : 1 ); comp++ ){
				if( comp )
					rmo_revcomp( buf.data(), slen );
				rmo_hits_t	oh;
				rmo_hits_init( &oh, pr.prog.get() );
				rmo_set_efn2data( pr.efn2.get() );
				rmo_scan( pr.prog.get(), pr.efn.get(), int( r ), buf.data(), slen, comp, &oh );
				BulkSeq	bs;
				bs.W = &W;
				bs.off = pf.base_off[ ent ];
				bs.slen = slen;
				bs.comp = comp;
				const CodeSeq	cs = bs;
				for( int64_t h = 0; h < oh.n; h++ ){
					const int32_t	*w = oh.data + h * stride;
					char	what[ 96 ];
					snprintf( what, sizeof( what ), "entry %zu comp %d hit %lld, window()", r, comp, ( long long )h );
					if( dp.efn_big )
						check_sites<BulkSeq, 1>( dp, pr, T16, facts, bs, w, w + n_cmp, what, &ss );
					else
						check_sites<BulkSeq, 0>( dp, pr, T16, facts, bs, w, w + n_cmp, what, &ss );
					snprintf( what, sizeof( what ), "entry %zu comp %d hit %lld, code()", r, comp, ( long long )h );
					if( dp.efn_big )
						check_sites<CodeSeq, 1>( dp, pr, T16, facts, cs, w, w + n_cmp, what, nullptr );
					else
						check_sites<CodeSeq, 0>( dp, pr, T16, facts, cs, w, w + n_cmp, what, nullptr );
					ss.cands++;
				}
				rmo_hits_free( &oh );
			}
		}
		free( W.codes );
		free( W.amask );
		printf( "%s: %lld candidates, %lld sites (%lld cached, %lld longer than the cache, %lld rejected), %lld mismatches\n",
			args.dfname.c_str(), ss.cands, ss.sites, ss.cached, ss.longer, ss.rejected, bad );
		return bad ? 1 : 0;
	}catch( rma::Error &e ){
		fprintf( stderr, "%s\n", e.what() );
		return 2;
	}
}
