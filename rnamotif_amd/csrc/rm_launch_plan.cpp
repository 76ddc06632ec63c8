// rm_launch_plan.cpp -- the launch shape of a scan (rm_launch_plan.h): host arithmetic only, no HIP call.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#define RMD_FN		static inline
#define RMD_FN_MEMBER	inline
#include "rm_launch_plan.h"

namespace rma {

static int env_int( const char *name, int dflt )
{
	const char	*v = getenv( name );
	return v != nullptr && v[ 0 ] != '\0' ? atoi( v ) : dflt;
}

void Options::latch()
{
	dbg = env_int( "RNAMOTIF_DBG", 0 );
	pool = env_int( "RNAMOTIF_POOL", -1 );
	pool_min = std::max( 1, env_int( "RNAMOTIF_POOL_MIN", 1024 ) );
	pool_refill = env_int( "RNAMOTIF_POOL_REFILL", 48 );
	drain = env_int( "RNAMOTIF_DRAIN", 1 );
	glist = env_int( "RNAMOTIF_GLIST", 0 );
	drain_waves = env_int( "RNAMOTIF_DRAIN_WAVES", 6 );
	search_wgs = env_int( "RNAMOTIF_SEARCH_WGS", 0 );
	set( "beside", env_int( "RNAMOTIF_BESIDE", -1 ) );
	struct_wgs = std::max( 0, env_int( "RNAMOTIF_STRUCT_WGS", 0 ) );
	flush = env_int( "RNAMOTIF_FLUSH", -1 );
	efn_light = env_int( "RNAMOTIF_EFN_LIGHT", -1 );
	host_sort = env_int( "RNAMOTIF_HOSTSORT", 0 );
	spec_tail = env_int( "RNAMOTIF_SPEC_TAIL", -1 );
	timing = getenv( "RNAMOTIF_TIMING" ) != nullptr;
	if( const char *f = getenv( "RNAMOTIF_SHORT" ) )
		short_force = f[ 0 ] == '1' ? 1 : f[ 0 ] == '2' ? 2 : 0;
	tile = env_int( "RNAMOTIF_TILE", 0 );
	if( tile < 0 || tile > 16384 )
		tile = 0;
	qcap = env_int( "RNAMOTIF_QCAP", 0 );
	spill = env_int( "RNAMOTIF_SPILL", -1 );
	budget = env_int( "RNAMOTIF_BUDGET", 0 );
}

bool Options::set( const std::string &n, int value )
{
	if( n == "dbg" ) dbg = value;
	else if( n == "pool" ) pool = value;
	else if( n == "pool_min" ) pool_min = std::max( 1, value );
	else if( n == "pool_refill" ) pool_refill = value;
	else if( n == "drain" ) drain = value;
	else if( n == "glist" ) glist = std::max( 0, value );
	else if( n == "drain_waves" ) drain_waves = std::max( 0, value );
	else if( n == "search_wgs" ) search_wgs = std::max( 0, value );
	else if( n == "beside" ) beside = value < 0 ? -1 : value != 0;
	else if( n == "struct_wgs" ) struct_wgs = std::max( 0, value );
	else if( n == "score_budget" ) score_budget = std::max( 1, value );
	else if( n == "score_heap" ) score_heap = std::min( std::max( 0, value ), 1 << 16 );
	else if( n == "flush" ) flush = value;
	else if( n == "efn_light" ) efn_light = value;
	else if( n == "host_sort" ) host_sort = value;
	else if( n == "spec_tail" ) spec_tail = value;
	else if( n == "timing" ) timing = value;
	else if( n == "short" ) short_force = value;
	else return false;
	return true;
}

size_t search_lds_bytes( int prog_bytes, const rmd_program_t &dp, int tile_t, bool lean, int qcap, int group, bool flush )
{
	const int	tile_bytes = tile_t + dp.w_winsize + dp.lmargin + dp.rmargin + 80;
	// (bit vectors of a tile: the literal's, five per pair-row set, four of a leading 4-plex' strand filter, five more when a triplex follows it)
	// (lean with a look-ahead chain: one more -- the start positions that remain; the chain's other vectors
	// borrow the place of the search records, which pass A does not use)
	// (... and five when the descriptor has a best literal: where each base stands, for the literal's occurrence vector)
	const size_t	pb_bytes = ( ( lean ? 6 + ( ( dp.chain.on || dp.lit_re >= 0 ) && group == 1 ? 1 : 0 ) : 1 + 5 * size_t( dp.n_rowsets ) + ( dp.q1f.on ? ( dp.q1f.t_on ? 9 : 4 ) : 0 ) + ( dp.lit_re >= 0 ? 1 : 0 ) ) +
			( dp.lit_re >= 0 && group == 1 ? 5 : 0 ) ) *
		( size_t( tile_bytes + 63 ) / 64 + 3 ) * sizeof( unsigned long long );
	size_t	lds = size_t( prog_bytes ) + size_t( qcap ) * sizeof( unsigned ) +
		size_t( group ) * ( ( ( size_t( tile_bytes ) + 15 ) & ~size_t( 15 ) ) + pb_bytes );
	// (the instance that walks nothing has no records: only the look-ahead chain's ten working vectors, which elsewhere borrow their place)
	if( flush )
		lds += dp.chain.on ? size_t( 10 ) * ( size_t( tile_bytes + 63 ) / 64 + 3 ) * sizeof( unsigned long long ) : 0;
	else
		lds += lean ? size_t( dp.n_searches ) * SEARCH_BLOCK * LEAN_REC_BYTES : size_t( dp.n_rec_dwords ) * GENERAL_BLOCK * 4;
	if( lean && group > 1 && dp.lit_re >= 0 )	// (groups: the literal's five vectors once per wave, behind the records)
		lds += 8 + size_t( SEARCH_BLOCK / 64 ) * 6 * ( size_t( tile_bytes + 63 ) / 64 + 3 ) * sizeof( unsigned long long );	// (the sixth: the literal's start positions)
	if( !lean && dp.split_s >= 0 )		// resume states of the levels up to the split level, queue of continuations
		lds += size_t( dp.split_s + 1 ) * GENERAL_BLOCK * 8 + size_t( DEEP_QUEUE ) * ( 2 + 2 * ( dp.split_s + 1 ) ) * 4;
	return lds;
}

// dwords of an item's window, four bits a base: what the pooled instances and the drain kernel lay out per lane
static int window_dwords( const rmd_program_t &dp ) { return ( dp.w_winsize + dp.lmargin + dp.rmargin + 14 ) / 8; }

// the largest tile of hi, hi - 256, ... down to lo that fits (0: none)
template< class Fits >
static int largest_tile( int hi, int lo, Fits fits )
{
	for( int t = hi; t >= lo; t -= 256 )
		if( fits( t ) )
			return t;
	return 0;
}

// Work queue items a start position yields on random sequence: n_rank * P( first minlen pairs hold, at most
// lim mispairs ) -- and only where the best literal occurs at an allowed offset.
static double queue_density( const rmd_program_t &dp )
{
	const rmd_elem_t	&e0 = dp.elems[ dp.searches[ 0 ] ];
	double	density = 1.0;
	if( e0.type == RMA_T_H5 && e0.pairset >= 0 && e0.minlen >= 1 ){
		const uint32_t	m2 = rmd_pairsets( &dp )[ e0.pairset ].mat2;
		int	np = 0;
		for( int a = 0; a < 4; a++ )
			for( int b = 0; b < 4; b++ )
				np += ( m2 >> ( a * 5 + b ) ) & 1;
		const double	pp = np / 16.0;
		const int	lim = ( e0.ends & RMA_5PAIRED ) ? e0.mplim : std::max( e0.mplim, 1 );
		double	p = 0, comb = 1;
		for( int m = 0; m <= lim && m <= e0.minlen; m++ ){
			p += comb * std::pow( pp, e0.minlen - m ) * std::pow( 1 - pp, m );
			comb = comb * ( e0.minlen - m ) / ( m + 1 );
		}
		const int	w = dp.w_winsize;
		const int	n_rank = ( e0.maxglen != RMA_UNBOUNDED && e0.maxglen < w ? e0.maxglen : w ) - e0.minglen + 1;
		density = std::min( 1.0, p ) * std::max( 1, n_rank );
	}
	if( dp.lit_re >= 0 ){
		const rmd_regex_t	&lre = rmd_regexes( &dp )[ dp.lit_re ];
		double	pl = 1.0;
		for( int j = 0; j < lre.n_states; j++ ){
			int	n = 0;
			for( int c = 0; c < 4; c++ )
				n += int( ( lre.accept[ c ] >> j ) & 1 );
			pl *= n / 4.0;
		}
		density *= std::min( 1.0, pl * ( dp.lit_hi - dp.lit_lo + 1 ) );
	}
	return density;
}

ProgramPlan plan_program( const rma_program_t &prog, const rmd_program_t &dp, int prog_bytes, int spill_cap, const Options &o )
{
	ProgramPlan	pp;
	pp.dp = &dp;
	pp.prog_bytes = prog_bytes;
	pp.strands = prog.chk_both_strs ? 2 : 1;
	pp.dminlen = prog.dminlen;
	for( int k = 0; k < dp.n_searches; k++ ){
		const rmd_elem_t	&e = dp.elems[ dp.searches[ k ] ];
		if( e.type == RMA_T_H5 && !e.proper )
			pp.kinds |= RMD_KIND_PK;
		if( e.type == RMA_T_P5 || e.type == RMA_T_T1 || e.type == RMA_T_Q1 )
			pp.kinds |= RMD_KIND_TQ;
	}
	if( dp.lean_ok ){
		// The search of a tile ends with a few long-running items on a few lanes, so fewer,
		// larger tiles are better as long as four workgroups still share a CU's 160 KB of LDS
		// (trna.descr, ms per 100 Mbase: T = 2048 6.97, 4096 5.87, 6144 5.40 with 8-byte records;
		// 6656 4.38, 9984 3.99 with 6-byte records; one step further only three fit: 5.0) and the
		// work queue still holds what the pre-filter lets through (queue_density).
		const double	density = queue_density( dp );
		// What the LDS queue cannot hold spills to HBM at 4 bytes per item, so LDS goes to the tile
		// first and the queue gets what is left, up to the expected number of items (trna.descr:
		// queue 1024 / T 9984 3.99 ms, 512 / 11008 3.94, 256 / 11520 3.91 -- the last spills a
		// third of its items for that 1 %: the queue starts at 512).  A tile should still not
		// produce more than half the spill area on average.
		const int	q_min = 512;
		// the largest tile from hi down that fits `budget` with the smallest queue (else `fallback`), and then the queue it leaves room for
		auto fit = [ & ]( int hi, size_t budget, bool flush, int fallback, int *tile, int *qcap ){
			*tile = largest_tile( hi, 2048, [ & ]( int t ){
				return search_lds_bytes( prog_bytes, dp, t, true, q_min, 1, flush ) <= budget &&
					density * t * 1.1 <= q_min + std::max( spill_cap, 2 * 512 ) / 2; } );
			*tile = *tile ? *tile : fallback;
			*qcap = q_min;
			const int	q_want = int( std::min( 8192.0, std::ceil( density * *tile * 1.2 / 256 ) * 256 ) );
			while( *tile > 0 && *qcap + 256 <= q_want && search_lds_bytes( prog_bytes, dp, *tile, true, *qcap + 256, 1, flush ) <= budget )
				*qcap += 256;
		};
		// (static __shared__: the waves' buffers of start positions that passed the look-ahead, 1 KB, and 40 bytes)
		fit( 16384, ( 160 * 1024 ) / SEARCH_WAVES_PER_SIMD - 1152, false, 2048, &pp.tile_t, &pp.qcap );
		// The pooled instance that walks nothing (RMK_LEAN_FLUSH: every survivor of pass A' goes to the drain kernel's list):
		// FLUSH_WAVES_PER_SIMD workgroups a CU, tiles as large as its smaller share of LDS holds without the search records.
		// For descriptors with a look-ahead chain -- a few dozen long walks per workgroup, which the drain kernel takes anyway;
		// hundreds of cheap items (ire.descr, mp.ends.descr) are walked best where they are found.
		// (pp.flush: it can run; use_flush(): the options of the moment want it)
		pp.flush = window_dwords( dp ) <= 32;
		if( pp.flush ){
			// (no larger than one pass of the workgroup's 256 lanes decodes, 32 bases a lane: profiles/flush_matrix.sh -- tiles of
			// 7936 positions 0.639 ms, of 8192, a second pass for ten lanes, 0.757; of 10752 0.658)
			const int	t_one = ( 254 * 32 - 61 - ( dp.w_winsize + dp.lmargin + dp.rmargin ) ) / 256 * 256;
			fit( std::max( 2048, std::min( 16384, t_one ) ), ( 160 * 1024 ) / FLUSH_WAVES_PER_SIMD - 1152, true, 0, &pp.tile_t_flush, &pp.qcap_flush );
			pp.flush = pp.tile_t_flush > 0;
		}
	}else{
		// general instance: workgroups of one wave (GENERAL_BLOCK), as many per SIMD as the registers allow
		// (GENERAL_WAVES) and as still leave every one of them a tile of a thousand positions or more next
		// to its records -- 12 bytes per level and lane -- and its queue (what the queue cannot hold spills
		// to HBM)
		const int	per_wave = SEARCH_BLOCK / GENERAL_BLOCK;	// workgroups where one of four waves stood
		pp.qcap = 512 / per_wave < 128 ? 128 : 512 / per_wave;
		pp.tile_t = 1024;
		// (descriptors with triplexes / 4-plexes: two workgroups per SIMD on tiles of three thousand positions
		// rather than three on a thousand -- a tile's second round then has a few dozen continuations for
		// its lanes instead of five: qu+tr 19.6 -> 16.7 ms; pk1 and pk_j1+2 are best at 2048, four per SIMD)
		for( int wg = ( pp.kinds & RMD_KIND_TQ ) ? 2 : GENERAL_WAVES( 0 ); wg >= 1; wg-- ){
			const size_t	budget = ( 160 * 1024 ) / ( wg * per_wave ) - ( per_wave > 1 ? 1024 : 2560 );	// (static __shared__ -- the pre-filter's wave buffers -- and allocation granules)
			const int	t = largest_tile( per_wave > 1 ? 4096 : 8192, wg > 1 ? 3072 / per_wave : 1024 / per_wave, [ & ]( int t ){
				return search_lds_bytes( prog_bytes, dp, t, false, pp.qcap ) <= budget; } );
			if( t > 0 ){
				pp.tile_t = t;
				break;
			}
		}
	}
	if( o.qcap >= 64 && o.qcap <= 16384 )
		pp.qcap = pp.qcap_flush = ( o.qcap + 3 ) & ~3;	// (what follows the queue in LDS is read 8 bytes at a time)
	if( o.tile > 0 )
		pp.tile_t = o.tile;
	return pp;
}

// the pooled instance that walks nothing: where it can run (plan_program) and the options do not ask for the other one
static bool use_flush( const ProgramPlan &pp, const Options &o )
{
	return pp.flush && o.drain != 0 && o.pool != 0 && !( o.dbg & ( RMK_DBG_GENERAL | RMK_DBG_POOL_DROP | RMK_DBG_LIST_ALL ) ) &&
		( o.flush < 0 ? pp.dp->chain.on != 0 : o.flush != 0 );
}

// the pooled lean instance (see the kernel): when the window of an item, four bits a base, fits the
// column a lane gets of the tile's place in LDS
static bool pooled_fits( const ProgramPlan &pp, const Options &o, int tile_t, bool flush = false )
{
	const rmd_program_t	&dp = *pp.dp;
	if( !dp.lean_ok || ( o.dbg & RMK_DBG_GENERAL ) )
		return false;
	if( flush )		// (the instance that walks nothing lays out no window: plan_program asked what the drain kernel asks)
		return use_flush( pp, o );
	const int	tile_bytes = tile_t + dp.w_winsize + dp.lmargin + dp.rmargin + 80;
	const int	n_dw = window_dwords( dp );
	const size_t	room = size_t( ( tile_bytes + 15 ) & ~15 ) + size_t( 6 + ( dp.chain.on ? 1 : 0 ) ) * ( ( tile_bytes + 63 ) / 64 + 3 ) * sizeof( unsigned long long );
	bool	pooled = n_dw <= 32 && size_t( n_dw ) * SEARCH_BLOCK * sizeof( uint32_t ) <= room;
	if( o.pool >= 0 )		// 0: pass B tile by tile (tests, profiles/pool_matrix.py)
		pooled = pooled && o.pool != 0;
	return pooled;
}

// The launch shape of a database.  Long entries: the program's tile, one per workgroup pass.  A database of
// many short entries (GenBank divisions, transcript sets) never fills such a tile, and a few dozen queue items
// cannot occupy 256 lanes: it gets small tiles in groups of SHORT_GROUP per workgroup pass
// (rma_search_kernel<.., G>), if the descriptor is lean and the group fits the LDS budget.
LayoutKey choose_layout( const ProgramPlan &pp, const Options &o, const DbShape &db, int cus )
{
	const rmd_program_t	&dp = *pp.dp;
	LayoutKey	k{ pp.tile_t, pp.dminlen, pp.strands, 1, pp.qcap };
	const int	n = db.n_seq;
	const bool	short_db = n >= 64 && db.sum_slen / n < SHORT_ENTRY_MEAN && o.tile == 0;
	// (cloverleaf-like descriptors -- a look-ahead chain whose first helix is tested jointly with the stem-loop behind
	// it -- do better tile by tile even there: chain, pass A' and the drain kernel are the one-tile instance's;
	// trna.descr over the reference's test database x 20: 3.36 against 3.70 ms.  bulge.descr, a chain of one
	// stem-loop, stays with the groups: 1.57 against 2.30.)
	bool	grouped = short_db && !( dp.chain.on && dp.chain.hn_on );
	if( o.short_force >= 0 )		// 0 never, 1 always (tests)
		grouped = o.short_force == 1;
	// Short entries and a descriptor the pooled instance takes: tiles over the concatenation of the entries (round 4)
	// -- whole start positions only (no slices), entries in order in the packed arrays, positions within 30 bits.
	k.concat = ( o.short_force < 0 ? short_db : o.short_force == 2 ) && n >= 1 &&
		!db.ranges && db.ascending && db.padded_bases < ( int64_t( 1 ) << 30 ) &&
		( pooled_fits( pp, o, k.tile_t ) || !dp.lean_ok || ( o.dbg & RMK_DBG_GENERAL ) ) && !dp.wide;		// (the pooled lean instance, or a general one)
	if( k.concat )
		grouped = false;
	// (long entries, a descriptor with a look-ahead chain: the instance that walks nothing, on tiles of its own size)
	k.flush = use_flush( pp, o ) && !grouped;
	if( k.flush ){
		k.tile_t = o.tile > 0 ? o.tile : pp.tile_t_flush;
		k.qcap = pp.qcap_flush;
	}
	if( grouped && dp.lean_ok && !( o.dbg & RMK_DBG_GENERAL ) ){
		const size_t	budget = ( 160 * 1024 ) / SEARCH_WAVES_PER_SIMD - 64 - SHORT_GROUP * 32;
		const int	q = o.qcap > 0 ? std::max( 64, o.qcap ) : 256;	// LDS goes to the slots; what a group queues beyond this spills (tests: force the overflow path)
		// (tiles of 1024 positions measured slower than of 768 where both fit: mp.ends 1.56 / 1.40 ms)
		const int	t = largest_tile( 768, 256, [ & ]( int t ){ return search_lds_bytes( pp.prog_bytes, dp, t, true, q, SHORT_GROUP ) <= budget; } );
		if( t > 0 ){
			k.tile_t = t;
			k.qcap = q;
			k.group = SHORT_GROUP;
		}
	}
	// A general instance's tile is one wave's, walks and all, for milliseconds: a database of fewer tiles than the device
	// holds workgroups (eight a CU) gets smaller ones -- down to 256 positions -- so that a short database, or one heavy
	// region of it, is not the work of a handful of waves (a 6 000 base database of repeats: 3 tiles, 90 s).
	if( !dp.lean_ok && k.group == 1 && o.tile == 0 ){
		const int64_t	positions = ( k.concat ? db.padded_bases : db.sum_slen ) * k.strands, slots = int64_t( cus ) * 8;
		if( positions / k.tile_t < slots )
			k.tile_t = int( std::min<int64_t>( k.tile_t, std::max<int64_t>( 256, ( positions / slots + 63 ) / 64 * 64 ) ) );
	}
	return k;
}

void make_tiling( const LayoutKey &k, const std::vector<int32_t> &slen, const std::vector<int64_t> &base_off,
	const std::vector<int32_t> &pos_lo, const std::vector<int32_t> &pos_hi, int64_t padded_bases, Tiling *out )
{
	Tiling	&l = *out;
	const int	n = int( slen.size() ), tile_t = k.tile_t, strands = k.strands;
	l.concat_bases = padded_bases;
	std::vector<int64_t>	&tile_start = l.h_tile_start;
	tile_start.assign( size_t( n ) + 1, 0 );
	if( k.concat ){
		// one "entry" of padded_bases bases per strand; a tile's line names the entries its start positions fall into
		// (RMK_META_SEQ: the first, RMK_META_PAD: how many -- the search of an item's entry stays within them)
		const int64_t	total = padded_bases, nsz = total - k.dminlen + 1;
		const int64_t	nt = nsz > 0 ? ( nsz + tile_t - 1 ) / tile_t : 0;
		l.n_tiles = nt * strands;
		tile_start[ n ] = l.n_tiles;		// (nothing reads the per-entry sums of such a tiling)
		l.h_tile_seq.assign( 1, 0 );
		std::vector<int32_t>	&meta = l.h_tile_meta;
		meta.assign( size_t( std::max<int64_t>( l.n_tiles, 1 ) ) * RMK_META_WORDS, 0 );
		auto entry_at = [ & ]( int64_t g ) -> int {	// the last entry that begins at or before base g of the arrays
			const int	e = int( std::upper_bound( base_off.begin(), base_off.end(), g ) - base_off.begin() ) - 1;
			return e < 0 ? 0 : e;
		};
		for( int64_t t = 0; t < l.n_tiles; t++ ){
			const int	comp = int( t / nt );
			const int64_t	z0 = ( t % nt ) * tile_t, z1 = std::min<int64_t>( z0 + tile_t, nsz ) - 1;
			const int64_t	g_lo = comp ? total - 1 - z1 : z0, g_hi = comp ? total - 1 - z0 : z1;
			const int	k_lo = entry_at( g_lo ), k_hi = entry_at( g_hi );
			int32_t	*m = &meta[ size_t( t ) * RMK_META_WORDS ];
			m[ RMK_META_SEQ ] = k_lo;
			m[ RMK_META_COMP ] = comp;
			m[ RMK_META_Z0 ] = int32_t( z0 );
			m[ RMK_META_SLEN ] = int32_t( total );
			m[ RMK_META_OFF_LO ] = m[ RMK_META_OFF_HI ] = 0;
			m[ RMK_META_POS_HI ] = 0x7fffffff;
			m[ RMK_META_PAD ] = k_hi - k_lo + 1;
		}
		return;
	}
	for( int i = 0; i < n; i++ ){
		int64_t	nsz = int64_t( slen[ i ] ) - k.dminlen + 1;	// start positions of a strand
		if( !pos_lo.empty() )
			nsz = std::min<int64_t>( nsz, pos_hi[ i ] ) - pos_lo[ i ];
		const int64_t	nt = nsz > 0 ? ( nsz + tile_t - 1 ) / tile_t : 0;
		tile_start[ i + 1 ] = tile_start[ i ] + nt * strands;
	}
	l.n_tiles = tile_start[ n ];
	l.h_tile_seq.resize( size_t( std::max<int64_t>( l.n_tiles, 1 ) ) );
	for( int i = 0; i < n; i++ )
		for( int64_t t = tile_start[ i ]; t < tile_start[ i + 1 ]; t++ )
			l.h_tile_seq[ size_t( t ) ] = i;
	if( k.group != 1 )
		return;
	l.h_tile_meta.assign( size_t( std::max<int64_t>( l.n_tiles, 1 ) ) * RMK_META_WORDS, 0 );
	for( int i = 0; i < n; i++ ){
		const int64_t	per_strand = ( tile_start[ i + 1 ] - tile_start[ i ] ) / strands;
		const int	lo = pos_lo.empty() ? 0 : pos_lo[ i ], hi = pos_hi.empty() ? 0x7fffffff : pos_hi[ i ];
		for( int64_t t = tile_start[ i ]; t < tile_start[ i + 1 ]; t++ ){
			int32_t	*m = &l.h_tile_meta[ size_t( t ) * RMK_META_WORDS ];
			const int64_t	local = t - tile_start[ i ];
			m[ RMK_META_SEQ ] = i;
			m[ RMK_META_COMP ] = int32_t( local / per_strand );
			m[ RMK_META_Z0 ] = lo + int32_t( local % per_strand ) * tile_t;
			m[ RMK_META_SLEN ] = slen[ i ];
			m[ RMK_META_OFF_LO ] = int32_t( uint64_t( base_off[ i ] ) & 0xffffffffu );
			m[ RMK_META_OFF_HI ] = int32_t( uint64_t( base_off[ i ] ) >> 32 );
			m[ RMK_META_POS_HI ] = hi;
		}
	}
}

// The instance that walks nothing, shaped so that the drain kernel of ANOTHER scanner's scan is sure of room beside it
// (option beside; two scanners that take the steps in turns).  Capping the grid at four workgroups a CU is not enough:
// at the hand-over two such kernels are in flight, five workgroups of any mix fit a CU, and a SIMD with five of their
// waves has 512 - 5 * 88 = 72 registers left where a drain wave needs 128 -- the grid is persistent, so such a CU is
// closed to the drain kernel for the whole launch.  So the dynamic LDS is padded until five do NOT fit, which holds for
// any mix of kernels planned this way, and the drain kernel gets as many waves a CU as find LDS beside four of them,
// one a SIMD at most (4 * 96 + 128 registers).  Instance, tiles and layout key stay: the kernel lays out its LDS from
// tile_bytes and prog_bytes and never asks how much there is, and both shapes share the database's tiling.
static void plan_beside( const Options &o, int cus, LaunchPlan *out )
{
	LaunchPlan	&p = *out;
	const size_t	cu_lds = 160 * 1024, SEARCH_STATIC_LDS = 1152;
	const int	wgs = FLUSH_WGS_PER_CU - 1;
	const size_t	lds = std::max( p.lds, ( cu_lds / FLUSH_WGS_PER_CU / 64 + 1 ) * 64 );	// (the instance's own, where that is more than a fifth already)
	// (what four of them take includes their static __shared__, the 1152 bytes plan_program() budgets for: three drain waves
	// of trna.descr's 10 400 bytes fit beside 4 * 32 832 on paper, two beside 4 * 33 984 on the device -- and a third that
	// waits for room only shrinks the shares of the two that run: 0.637 against 0.619 ms a step)
	const size_t	taken = wgs * ( lds + SEARCH_STATIC_LDS );
	const size_t	left = cu_lds > taken ? cu_lds - taken : 0;
	const int	n = int( std::min<size_t>( std::min( o.drain_waves > 0 ? o.drain_waves : 16, 4 ), left / ( p.drain_lds + 64 ) ) );
	if( n < 2 )		// (no room worth the fifth workgroup: the solo shape)
		return;
	p.lds = lds;
	p.grid = std::min( p.grid, wgs * cus );
	p.drain_grid = cus * n;
	p.beside = true;
}

int plan_launch( const LayoutKey &k, int64_t n_tiles, const ProgramPlan &pp, const Options &o, int cus, LaunchPlan *out,
	char *err, size_t errlen )
{
	const rmd_program_t	&dp = *pp.dp;
	LaunchPlan	&p = *out;
	p = LaunchPlan();
	const int	grid_blocks = cus * 8;		// most workgroups of a launch of a lean instance (eight of four waves per CU)
	p.lean = dp.lean_ok && !( o.dbg & RMK_DBG_GENERAL );
	p.grouped = p.lean && k.group > 1;
	p.tile_bytes = k.tile_t + dp.w_winsize + dp.lmargin + dp.rmargin + 80;
	p.lds = search_lds_bytes( pp.prog_bytes, dp, k.tile_t, p.lean, k.qcap, p.grouped ? SHORT_GROUP : 1, p.lean && k.flush );
	if( p.lds > 150 * 1024 ){
		snprintf( err, errlen, "window of %d bases does not fit the LDS tile (%zu bytes needed)", dp.w_winsize, p.lds );
		return 1;
	}
	p.pooled = p.lean && !p.grouped && pooled_fits( pp, o, k.tile_t, k.flush );
	if( k.concat && p.lean && !p.pooled ){
		snprintf( err, errlen, "a tiling over the concatenation of the entries is for the pooled lean instance and the general ones" );	// (choose_layout asks pooled_fits too)
		return 1;
	}
	if( p.pooled ){
		// the drain kernel: one wave per workgroup -- the program, a window column and the records of 64 lanes
		p.drain_nib = window_dwords( dp );	// (at most 32: pooled_fits)
		p.drain_lds = size_t( pp.prog_bytes ) + size_t( p.drain_nib + dp.n_searches ) * 64 * sizeof( uint32_t ) + size_t( dp.n_searches ) * 64 * sizeof( uint16_t );
		const int	per_cu = int( std::min<size_t>( 4 * SEARCH_WAVES_PER_SIMD, ( 160 * 1024 ) / ( p.drain_lds + 64 ) ) );
		p.drain_grid = cus * std::max( 1, o.drain_waves > 0 ? std::min( o.drain_waves, per_cu ) : per_cu );
	}
	// the kernel instance: lean (pooled, one tile or a group of small ones per pass), or the general one
	// compiled for the kinds of element the descriptor has
	const int	kinds = pp.kinds;
	p.inst = p.pooled ? ( k.concat ? ( k.flush ? RMK_LEAN_CONCAT_FLUSH : RMK_LEAN_CONCAT ) : k.flush ? RMK_LEAN_FLUSH : RMK_LEAN_POOL ) :
		p.grouped ? RMK_LEAN_GROUP : p.lean ? RMK_LEAN_TILE : dp.wide ? RMK_GEN_WIDE :
		k.concat ? ( kinds == 0 ? RMK_GEN_PLAIN_CONCAT : kinds == RMD_KIND_PK ? RMK_GEN_PK_CONCAT : kinds == RMD_KIND_TQ ? RMK_GEN_TQ_CONCAT : RMK_GEN_PKTQ_CONCAT ) :
		kinds == 0 ? RMK_GEN_PLAIN : kinds == RMD_KIND_PK ? RMK_GEN_PK : kinds == RMD_KIND_TQ ? RMK_GEN_TQ : RMK_GEN_PKTQ;
	p.listed = p.pooled;		// (the four pooled instances)
	p.walks_nothing = p.inst == RMK_LEAN_FLUSH || p.inst == RMK_LEAN_CONCAT_FLUSH;
	const int64_t	n_units = p.grouped ? ( n_tiles + SHORT_GROUP - 1 ) / SHORT_GROUP : n_tiles;
	p.grid = int( std::min<int64_t>( n_units, p.lean ? grid_blocks : grid_blocks * wgs_per_wave( dp ) ) );
	if( p.lean && o.search_wgs > 0 )		// (option search_wgs: workgroups of a lean search kernel per CU -- room for another scanner's drain kernel beside it)
		p.grid = std::min( p.grid, o.search_wgs * cus );
	else if( p.walks_nothing )
		// The instance that walks nothing is compiled for five workgroups a CU (96 registers, a fifth of the LDS) and runs
		// FLUSH_WGS_PER_CU = 5: option search_wgs at 3, 4 and 5 gives 0.900, 0.714 and 0.611 ms (trna.descr over 100 x 1 Mbase) --
		// every wave more hides other waves' waits.
		p.grid = std::min( p.grid, FLUSH_WGS_PER_CU * cus );
	// (behind the search instance that walks nothing: workgroups of one wave that find room next to another scanner's search
	// kernel -- the staged form's 136 KB of LDS wait until that kernel is through)
	p.efn_light = !dp.efn_big && ( o.efn_light < 0 ? p.walks_nothing : o.efn_light != 0 );
	if( o.beside == 1 && p.walks_nothing )
		plan_beside( o, cus, &p );
	return 0;
}

}	// namespace rma
