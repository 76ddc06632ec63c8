// rm_scanner.cpp -- the scanner / database half of the C ABI (include/rnamotif_amd.h) on the
// host: device memory, streams, the launches.  Their shapes are chosen in rm_launch_plan.cpp; the
// kernels are in rm_scan_kernel.h, reached through the launchers of rm_kernels.h.
//
// What belongs to whom:
//   DevCtx (one per GPU)  the upload stream and a cache of device blocks: a database that is
//                         destroyed gives its block back, the next one of about that size takes
//                         it -- no hipMalloc / hipFree per database (the loop over batches of the
//                         command line, rnamot.c:158-185, makes one per batch); it lives as long
//                         as the process
//   rma_db                the packed bases of some entries in HBM -- codes, ambiguity mask,
//                         offsets, lengths, start-position ranges: nothing in it depends on a
//                         descriptor -- plus, per launch shape that has scanned it, the tiling
//                         (tile_start / tile_seq), made when a scanner first meets the database
//   rma_scanner           the motif program of one descriptor on one GPU, its stream, hit buffer,
//                         work areas and ordering stage
// A database is uploaded on the device's upload stream; a scan waits for that on its own stream
// (an event), so the upload of the next database runs under the scan of this one.
// The two structs are defined in rm_scanner_impl.h, which also says who frees what and when (the
// owners are rm_hip_own.h's); the calls that consume records already on the
// device (windows, structures, alignments, pruning) are rm_hitpost.cpp's.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <set>

#define RMD_FN		static inline
#define RMD_FN_MEMBER	inline
#include "rm_scanner_impl.h"
#include "rm_scan_report.h"
#include "rm_efn_core.h"
#include "rm_efndata.h"
#include "rm_fasta.h"
#include "rm_pack.h"
#include "rm_dbpack_dev.h"
#include "rm_dbtext_dev.h"
#include "rm_fasta_dev_kernels.h"
#include "rm_stream.h"

using rma::Block;

// ---------------------------------------------------------------- per-device context
struct rma::DevCtx {
	int	device = 0;
	std::mutex	mu;
	rma::Stream	upload;
	std::vector<Block>	spare;		// blocks of destroyed databases, waiting for the next one
	size_t	spare_bytes = 0;
	// Take a block of at least `bytes`: a spare one that is not more than twice that, else a new one.
	hipError_t	take( size_t bytes, Block *out )
	{
		bytes = std::max<size_t>( ( bytes + 255 ) & ~size_t( 255 ), 256 );
		{
			std::lock_guard<std::mutex>	lk( mu );
			int	best = -1;
			for( size_t i = 0; i < spare.size(); i++ )
				if( spare[ i ].bytes >= bytes && spare[ i ].bytes <= 2 * bytes + ( 1 << 20 ) &&
					( best < 0 || spare[ i ].bytes < spare[ size_t( best ) ].bytes ) )
					best = int( i );
			if( best >= 0 ){
				*out = spare[ size_t( best ) ];
				spare_bytes -= out->bytes;
				spare.erase( spare.begin() + best );
				return hipSuccess;
			}
		}
		// (a little head room: the batches of one search differ by an entry or two)
		const size_t	want = bytes + bytes / 16;
		hipError_t	e = hipMalloc( &out->p, want );
		if( e != hipSuccess ){
			// the spare blocks are memory too: give them back and try again
			drop_spare();
			( void )hipGetLastError();
			e = hipMalloc( &out->p, want );
		}
		out->bytes = e == hipSuccess ? want : 0;
		return e;
	}
	void	give( Block b )
	{
		if( b.p == nullptr )
			return;
		{
			std::lock_guard<std::mutex>	lk( mu );
			// at most eight blocks and 4 GB wait here
			if( spare.size() < 8 && spare_bytes + b.bytes <= ( size_t( 4 ) << 30 ) ){
				spare.push_back( b );
				spare_bytes += b.bytes;
				return;
			}
		}
		( void )hipFree( b.p );
	}
	void	drop_spare()
	{
		std::lock_guard<std::mutex>	lk( mu );
		for( Block &b : spare )
			( void )hipFree( b.p );
		spare.clear();
		spare_bytes = 0;
	}
};
using rma::DevCtx;

namespace {

std::mutex	g_ctx_mu;
std::vector<DevCtx *>	g_ctx;		// (never destroyed: no call of the runtime is made while the process exits)

// (the caller has made `device` current)
DevCtx *dev_ctx( int device, char *err, size_t errlen )
{
	std::lock_guard<std::mutex>	lk( g_ctx_mu );
	for( DevCtx *c : g_ctx )
		if( c->device == device )
			return c;
	std::unique_ptr<DevCtx>	c( new DevCtx );
	c->device = device;
	hipError_t	e = c->upload.create( hipStreamNonBlocking );
	if( e != hipSuccess ){
		snprintf( err, errlen, "hipStreamCreate (upload stream): %s", hipGetErrorString( e ) );
		return nullptr;
	}
	g_ctx.push_back( c.release() );
	return g_ctx.back();
}

}	// namespace

// the tiling of a database for one launch shape, on the host and (blk) on the device
struct rma::Layout : rma::LayoutKey, rma::Tiling {
	Block	blk;
	int64_t	*d_tile_start = nullptr;
	int32_t	*d_tile_seq = nullptr;
	int32_t	*d_tile_meta = nullptr;
	rma::Event	ready;		// the copies are complete: every scan waits for it on its stream
};
using rma::Layout;

// the databases rma_db_create_device() has made and rma_db_destroy() has not yet destroyed (rma_replay_device
// refuses any other)
static std::mutex	g_device_dbs_mu;
static std::set<const rma_db *>	g_device_dbs;

bool rma::is_device_db( const rma_db *db )
{
	std::lock_guard<std::mutex>	lk( g_device_dbs_mu );
	return g_device_dbs.count( db ) != 0;
}

// every database that has been made and not yet destroyed (rma_db_text_attach refuses any other); under g_device_dbs_mu
static std::set<const rma_db *>	g_live_dbs;

static bool is_live_db( const rma_db *db )
{
	std::lock_guard<std::mutex>	lk( g_device_dbs_mu );
	return g_live_dbs.count( db ) != 0;
}

hipStream_t rma::upload_stream( const rma_db *db )
{
	return db->ctx->upload.get();
}

extern "C" void rma_db_destroy( rma_db_t *db );
extern "C" void rma_scanner_destroy( rma_scanner_t *sc );
extern "C" int rma_scan_end( rma_scanner_t *sc, const int32_t **hits, int64_t *n_hits, char *err, size_t errlen );

// a scanner / a database under construction: destroyed on every way out but release()
using ScannerPtr = std::unique_ptr<rma_scanner, void ( * )( rma_scanner * )>;
using DbPtr = std::unique_ptr<rma_db, void ( * )( rma_db * )>;

extern "C" int rma_device_count( void )
{
	int	n = 0;
	if( hipGetDeviceCount( &n ) != hipSuccess )
		return 0;
	return n;
}

hipError_t rmk_launch_search( int inst, int grid, size_t lds, hipStream_t s, const rmk_search_args &a )
{
	switch( inst ){
	case RMK_LEAN_POOL :	return rmk_launch_lean_pool( grid, lds, s, a );
	case RMK_LEAN_CONCAT :	return rmk_launch_lean_concat( grid, lds, s, a );
	case RMK_LEAN_FLUSH :	return rmk_launch_lean_flush( grid, lds, s, a );
	case RMK_LEAN_CONCAT_FLUSH :	return rmk_launch_lean_concat_flush( grid, lds, s, a );
	case RMK_LEAN_GROUP :	return rmk_launch_lean_group( grid, lds, s, a );
	case RMK_LEAN_TILE :	return rmk_launch_lean_tile( grid, lds, s, a );
	case RMK_GEN_PLAIN :	return rmk_launch_gen_plain( grid, lds, s, a );
	case RMK_GEN_PK :	return rmk_launch_gen_pk( grid, lds, s, a );
	case RMK_GEN_TQ :	return rmk_launch_gen_tq( grid, lds, s, a );
	case RMK_GEN_PKTQ :	return rmk_launch_gen_pktq( grid, lds, s, a );
	case RMK_GEN_WIDE :	return rmk_launch_gen_wide( grid, lds, s, a );
	case RMK_GEN_PLAIN_CONCAT :	return rmk_launch_gen_plain_concat( grid, lds, s, a );
	case RMK_GEN_PK_CONCAT :	return rmk_launch_gen_pk_concat( grid, lds, s, a );
	case RMK_GEN_TQ_CONCAT :	return rmk_launch_gen_tq_concat( grid, lds, s, a );
	case RMK_GEN_PKTQ_CONCAT :	return rmk_launch_gen_pktq_concat( grid, lds, s, a );
	}
	return hipErrorInvalidValue;
}

extern "C" int rma_scanner_create( const rma_program_t *prog, const rma_efndata_t *efn, int device,
	rma_scanner_t **out, char *err, size_t errlen )
{
	*out = nullptr;
	ScannerPtr	guard( new rma_scanner, rma_scanner_destroy );
	rma_scanner	*sc = guard.get();
	memcpy( &sc->prog, prog, sizeof( rma_program_t ) );	// (every byte, padding too: rma_score_hits compares the bytes with an image's copy)
	sc->opt.latch();
	// (host work first: a descriptor outside the device limits is refused with its reason whether
	// or not a device is there to refuse it for)
	if( rmd_build( prog, &sc->dprog, err, errlen ) )
		return 1;
	int	ndev = 0;
	if( hipGetDeviceCount( &ndev ) != hipSuccess || ndev <= 0 ){
		snprintf( err, errlen, "no HIP device available: the rnamotif scan path runs on the GPU only" );
		return 1;
	}
	if( device < 0 || device >= ndev ){
		snprintf( err, errlen, "device %d out of range (0..%d)", device, ndev - 1 );
		return 1;
	}
	if( sc->opt.budget > 0 )		// launch-shape switch: iterations per step
		sc->dprog.step_budget = std::max( 4, sc->opt.budget );
	for( int k = 0; k < prog->n_efn_sites; k++ ){
		if( prog->efn_sites[ k ].kind == RMA_EFN_KIND_EFN2 )
			sc->need_efn2 = true;	// tables come with rma_scanner_set_efn2data(), checked at the first scan
		else if( efn == nullptr ){
			snprintf( err, errlen, "the program has efn() call sites but no energy tables were given" );
			return 1;
		}
	}
	sc->device = device;
	HIPCHK( hipSetDevice( device ) );
	sc->ctx = dev_ctx( device, err, errlen );
	if( sc->ctx == nullptr )
		return 1;
	HIPCHK( sc->stream.create( hipStreamNonBlocking ) );
	for( int i = 0; i < 5; i++ )
		HIPCHK( sc->ev[ i ].create( hipEventDefault ) );
	{
		// the device gets the compact image; sc->dprog stays the full struct for the host
		std::vector<char>	img( sizeof( rmd_program_t ) );
		sc->prog_bytes = int( rmd_make_image( &sc->dprog, img.data() ) );
		HIPCHK( sc->d_prog.exact( size_t( sc->prog_bytes ) ) );
		HIPCHK( hipMemcpy( sc->d_prog.as<void>(), img.data(), size_t( sc->prog_bytes ), hipMemcpyHostToDevice ) );
	}
	HIPCHK( sc->d_counters.exact( RMK_N_COUNTERS * sizeof( unsigned long long ) ) );
	if( efn != nullptr && rma::efn_tables_to_device( sc, efn, err, errlen ) )
		return 1;
	hipDeviceProp_t	prop;
	HIPCHK( hipGetDeviceProperties( &prop, device ) );
	sc->grid_blocks = prop.multiProcessorCount * 8;
	// (the general instances run workgroups of one wave, four times as many, on tiles a quarter the size)
	sc->spill_blocks = sc->grid_blocks * rma::wgs_per_wave( sc->dprog );
	const int	spill = sc->opt.spill >= 0 ? sc->opt.spill : SPILL_ITEMS / rma::wgs_per_wave( sc->dprog );	// (tests: 0 = overflow searched in place)
	HIPCHK( sc->d_spill.exact( std::max<size_t>( size_t( sc->spill_blocks ) * spill, 1 ) * sizeof( unsigned ) ) );
	sc->plan = rma::plan_program( *prog, sc->dprog, sc->prog_bytes, sc->spill_cap(), sc->opt );
	// room for the candidates of a few hundred Mbase at the densities of the reference's descriptors
	// (63 per Mbase for trna.descr); a scan that finds more is repeated into a buffer of the right
	// size (count-then-emit, rma_scan_end)
	HIPCHK( sc->d_hits.exact( ( size_t( 1 ) << 17 ) * sc->dprog.hit_stride * sizeof( int32_t ) ) );
	HIPCHK( sc->h_ctr.exact( ( RMK_C_COPIED + 1 ) * sizeof( unsigned long long ) ) );
	// page-locked room for the records of a usual batch (16 K of them) now, not in the first scan
	HIPCHK( sc->h_raw.exact( size_t( 16384 ) * sc->dprog.hit_stride * sizeof( int32_t ) ) );
	if( sc->dsort.reserve( sc->hit_cap(), sc->dprog.hit_stride ) != hipSuccess )
		( void )hipGetLastError();	// (no room for the ordering's buffers: rma_scan_end orders on the host)
	*out = guard.release();
	return 0;
}

// efn()'s tables as the kernels read them.  Tables loaded again replace the ones that are there, in place; have_efn
// says that all three are complete.
int rma::efn_tables_to_device( rma_scanner *sc, const rma_efndata_t *efn, char *err, size_t errlen )
{
	std::vector<int16_t>	t16;
	std::vector<int32_t>	tlkey;
	rma::efn_tables16( efn, t16, tlkey );
	const struct { rma::DevMem *d; const void *h; size_t bytes; }	tables[ 3 ] = {
		{ &sc->d_t16, t16.data(), t16.size() * sizeof( int16_t ) },
		{ &sc->d_tlkey, tlkey.data(), tlkey.size() * sizeof( int32_t ) },
		{ &sc->d_loginc, efn->loginc, RMA_EFN_LOGINC * sizeof( int32_t ) } };
	sc->have_efn = false;
	for( const auto &t : tables ){
		if( t.d->bytes() < t.bytes )
			HIPCHK( t.d->exact( t.bytes ) );
		HIPCHK( hipMemcpy( t.d->as<void>(), t.h, t.bytes, hipMemcpyHostToDevice ) );
	}
	sc->have_efn = true;
	return 0;
}

extern "C" int rma_scanner_set_option( rma_scanner_t *sc, const char *name, int value, char *err, size_t errlen )
{
	const std::string	n = name ? name : "";
	if( n == "forget_last" ){
		// (not a switch: the last scan's records are no longer there for rma_gather_hits() -- a rank whose share of a
		// round is empty sends nothing, whatever the round before left)
		sc->d_last = nullptr;
		sc->n_last = 0;
		sc->last_state = 0;
		sc->last_relabelled = false;
	}else if( !sc->opt.set( n, value ) ){
		snprintf( err, errlen, "rma_scanner_set_option: no option '%s' that can change after creation "
			"(dbg, pool, pool_min, pool_refill, drain, glist, drain_waves, search_wgs, beside, struct_wgs, score_budget, score_heap, flush, efn_light, host_sort, spec_tail, timing, short; forget_last)", n.c_str() );
		return 1;
	}
	return 0;
}

extern "C" int rma_scanner_set_efn2data( rma_scanner_t *sc, const rma_efn2data_t *efn2, char *err, size_t errlen )
{
	HIPCHK( hipSetDevice( sc->device ) );
	rma::DevMem	fresh;		// (the scanner has tables once they are complete)
	rma::DevMem	&d = sc->d_efn2 ? sc->d_efn2 : fresh;
	if( !d )
		HIPCHK( d.exact( sizeof( rma_efn2data_t ) ) );
	HIPCHK( hipMemcpy( d.as<void>(), efn2, sizeof( rma_efn2data_t ), hipMemcpyHostToDevice ) );
	if( fresh )
		sc->d_efn2 = std::move( fresh );
	return 0;
}

extern "C" void rma_scanner_destroy( rma_scanner_t *sc )
{
	if( sc == nullptr )
		return;
	if( sc->stream.get() != nullptr ){	// (else: refused before anything was set up on a device)
		( void )hipSetDevice( sc->device );
		if( sc->fly.db != nullptr ){		// (a scan begun and never ended)
			const int32_t	*h = nullptr;
			int64_t	n = 0;
			char	e[ 256 ];
			( void )rma_scan_end( sc, &h, &n, e, sizeof( e ) );
		}
		( void )hipStreamSynchronize( sc->stream.get() );
		rma::hitpost_free( sc->post );		// (waits for its scratch stream first)
	}
	delete sc;
}

// ---------------------------------------------------------------- databases
// A database of n entries in a block of its own, the small tables -- base_off[] (the entries' offsets in
// bases, multiples of 32, in the device arrays), slen, pos_lo / pos_hi -- on their way on the device's
// upload stream; the packed words (n_mask mask words, twice as many code words) are the caller's to fill,
// on that stream, before db_ready().  extra: bytes of room past the tables (db_from_device's inputs), at
// *extra_at.
static int db_alloc( int device, const int64_t *base_off, const int32_t *slen, int32_t n, const int32_t *pos_lo, const int32_t *pos_hi,
	size_t n_mask, size_t extra, rma_db_t **out, char **extra_at, char *err, size_t errlen )
{
	*out = nullptr;
	if( pos_lo != nullptr )
		for( int i = 0; i < n; i++ )
			if( pos_lo[ i ] < 0 || pos_hi[ i ] < pos_lo[ i ] ){
				snprintf( err, errlen, "entry %d: start positions [%d, %d) are not a range", i, pos_lo[ i ], pos_hi[ i ] );
				return 1;
			}
	HIPCHK( hipSetDevice( device ) );
	DevCtx	*ctx = dev_ctx( device, err, errlen );
	if( ctx == nullptr )
		return 1;
	// every early return below frees what has been allocated so far
	DbPtr	guard( new rma_db, rma_db_destroy );
	rma_db	*db = guard.get();
	{
		std::lock_guard<std::mutex>	lk( g_device_dbs_mu );
		g_live_dbs.insert( db );
	}
	db->device = device;
	db->ctx = ctx;
	db->n_seq = n;
	db->h_slen.assign( slen, slen + n );
	db->h_base_off.assign( base_off, base_off + n );
	if( pos_lo != nullptr ){
		db->h_pos_lo.assign( pos_lo, pos_lo + n );
		db->h_pos_hi.assign( pos_hi, pos_hi + n );
	}
	for( int i = 0; i < n; i++ ){
		db->sum_slen += slen[ i ];
		db->max_slen = std::max( db->max_slen, slen[ i ] );
		if( pos_lo != nullptr )		// this database answers for a slice of the entry's start positions only
			db->total_bases += std::max<int64_t>( 0, std::min<int64_t>( pos_hi[ i ], slen[ i ] ) - pos_lo[ i ] );
		else
			db->total_bases += slen[ i ];
	}
	db->padded_bases = int64_t( n_mask ) * 32;
	for( int i = 0; i < n; i++ )
		if( base_off[ i ] < 0 || base_off[ i ] + slen[ i ] > db->padded_bases || ( i + 1 < n && base_off[ i ] + slen[ i ] > base_off[ i + 1 ] ) )
			db->ascending = false;
	// (carved twice: for the block's size, then in the block)
	auto	carve = [ & ]( void *base ){
		const size_t	nn = size_t( std::max( n, 1 ) );
		Carver	c;
		db->d_codes = c.take<uint32_t>( base, std::max<size_t>( 2 * n_mask, 1 ) );
		db->d_amask = c.take<uint32_t>( base, std::max<size_t>( n_mask, 1 ) );
		db->d_base_off = c.take<int64_t>( base, nn );
		db->d_slen = c.take<int32_t>( base, nn );
		if( pos_lo != nullptr ){
			db->d_pos_lo = c.take<int32_t>( base, nn );
			db->d_pos_hi = c.take<int32_t>( base, nn );
		}
		if( extra_at != nullptr )
			*extra_at = c.take<char>( base, 0 );
		return c.at;
	};
	const size_t	total = carve( nullptr ) + extra;
	HIPCHK( ctx->take( total, &db->blk ) );
	carve( db->blk.p );
	HIPCHK( db->ready.create( hipEventDisableTiming ) );
	hipStream_t	up = ctx->upload.get();
	if( n > 0 ){
		// (the small tables come from the host copies the database keeps: they outlive the call)
		HIPCHK( hipMemcpyAsync( db->d_base_off, db->h_base_off.data(), size_t( n ) * 8, hipMemcpyHostToDevice, up ) );
		HIPCHK( hipMemcpyAsync( db->d_slen, db->h_slen.data(), size_t( n ) * 4, hipMemcpyHostToDevice, up ) );
		if( pos_lo != nullptr ){
			HIPCHK( hipMemcpyAsync( db->d_pos_lo, db->h_pos_lo.data(), size_t( n ) * 4, hipMemcpyHostToDevice, up ) );
			HIPCHK( hipMemcpyAsync( db->d_pos_hi, db->h_pos_hi.data(), size_t( n ) * 4, hipMemcpyHostToDevice, up ) );
		}
	}
	*out = guard.release();
	return 0;
}

// The words of db are on their way on the upload stream: db->ready behind them (wait: until they are in).
// On failure db is destroyed.
static int db_ready( rma_db_t **out, bool wait, char *err, size_t errlen )
{
	DbPtr	guard( *out, rma_db_destroy );
	*out = nullptr;
	HIPCHK( hipEventRecord( guard->ready.get(), guard->ctx->upload.get() ) );
	if( wait )
		HIPCHK( hipEventSynchronize( guard->ready.get() ) );
	*out = guard.release();
	return 0;
}

// Upload n packed entries: `pieces` are runs of whole words of the source arrays that follow each
// other in the device arrays (one run for a slice of a pack, one per entry for chosen entries);
// base_off[] are the entries' offsets in bases (multiples of 32) in the device arrays.  wait:
// return when the copies are complete (the source may then go away); otherwise the caller keeps
// the source as it is until rma_db_wait() or the end of the first scan.
struct Piece { const uint32_t *codes, *amask; size_t mask_words; };

static int db_upload( int device, const std::vector<Piece> &pieces, const int64_t *base_off, const int32_t *slen, int32_t n,
	const int32_t *pos_lo, const int32_t *pos_hi, bool wait, rma_db_t **out, char *err, size_t errlen )
{
	size_t	n_mask = 0;
	for( const Piece &p : pieces )
		n_mask += p.mask_words;
	if( db_alloc( device, base_off, slen, n, pos_lo, pos_hi, n_mask, 0, out, nullptr, err, errlen ) )
		return 1;
	DbPtr	guard( *out, rma_db_destroy );
	rma_db	*db = guard.get();
	*out = nullptr;
	hipStream_t	up = db->ctx->upload.get();
	size_t	at = 0;		// mask words uploaded so far
	for( const Piece &p : pieces ){
		if( p.mask_words == 0 )
			continue;
		HIPCHK( hipMemcpyAsync( db->d_codes + 2 * at, p.codes, 2 * p.mask_words * 4, hipMemcpyHostToDevice, up ) );
		HIPCHK( hipMemcpyAsync( db->d_amask + at, p.amask, p.mask_words * 4, hipMemcpyHostToDevice, up ) );
		at += p.mask_words;
	}
	*out = guard.release();
	return db_ready( out, wait, err, errlen );
}

// the device a database made for scanner sc lives on (sc may be null: device 0)
static int device_of( const rma_scanner_t *sc ) { return sc != nullptr ? sc->device : 0; }

static const Layout *layout_for( rma_scanner_t *sc, const rma_db_t *cdb, char *err, size_t errlen, hipStream_t on = nullptr );

// a database made for a scanner gets that scanner's tiling with it, behind its words on the upload stream
static int tile_at_creation( rma_scanner_t *sc, rma_db_t **out, char *err, size_t errlen )
{
	if( sc == nullptr || layout_for( sc, *out, err, errlen, ( *out )->ctx->upload.get() ) != nullptr )
		return 0;
	rma_db_destroy( *out );
	*out = nullptr;
	return 1;
}

static int db_from_text( rma_scanner_t *sc, const char *const *seqs, const int32_t *slens, const int32_t *pos_lo, const int32_t *pos_hi,
	int32_t n, rma_db_t **out, char *err, size_t errlen )
{
	*out = nullptr;
	rma::PackedDb	pk;
	for( int i = 0; i < n; i++ )
		pk.add( seqs[ i ], slens[ i ] < 0 ? 0 : slens[ i ] );
	std::vector<Piece>	pieces{ Piece{ pk.codes.data(), pk.amask.data(), pk.amask.size() } };
	if( db_upload( device_of( sc ), pieces, pk.base_off.data(), pk.slen.data(), n, pos_lo, pos_hi, true, out, err, errlen ) )
		return 1;
	return tile_at_creation( sc, out, err, errlen );
}

extern "C" int rma_db_create_ranges( rma_scanner_t *sc, const char *const *seqs, const int32_t *slens,
	const int32_t *pos_lo, const int32_t *pos_hi, int32_t n, rma_db_t **out, char *err, size_t errlen )
{
	return db_from_text( sc, seqs, slens, pos_lo, pos_hi, n, out, err, errlen );
}

extern "C" int rma_db_create( rma_scanner_t *sc, const char *const *seqs, const int32_t *slens, int32_t n,
	rma_db_t **out, char *err, size_t errlen )
{
	return db_from_text( sc, seqs, slens, nullptr, nullptr, n, out, err, errlen );
}

const rma::PackFile *rma_pack_file( const rma_pack_t *pk );	// rm_capi.cpp

static int db_from_pack( rma_scanner_t *sc, const rma_pack_t *pack, int32_t first, int32_t count, bool wait,
	rma_db_t **out, char *err, size_t errlen )
{
	*out = nullptr;
	const rma::PackFile	&pf = *rma_pack_file( pack );
	if( first < 0 || count < 0 || first + count > pf.count() ){
		snprintf( err, errlen, "entries [%d, %d) are outside the packed database (%d entries)", first, first + count, pf.count() );
		return 1;
	}
	std::vector<Piece>	pieces;
	std::vector<int64_t>	rel( static_cast<size_t>( count ), 0 );
	if( count > 0 ){
		const int64_t	b0 = pf.base_off[ first ];
		const int	last = first + count - 1;
		const int64_t	b1 = pf.base_off[ last ] + ( ( int64_t( pf.slen[ last ] ) + 31 ) / 32 ) * 32;
		for( int i = 0; i < count; i++ )
			rel[ i ] = pf.base_off[ first + i ] - b0;
		pieces.push_back( Piece{ pf.codes.data() + b0 / 16, pf.amask.data() + b0 / 32, size_t( ( b1 - b0 ) / 32 ) } );
	}
	if( db_upload( device_of( sc ), pieces, rel.data(), pf.slen.data() + first, count, nullptr, nullptr, wait, out, err, errlen ) )
		return 1;
	return tile_at_creation( sc, out, err, errlen );
}

extern "C" int rma_db_create_packed( rma_scanner_t *sc, const rma_pack_t *pack, int32_t first, int32_t count,
	rma_db_t **out, char *err, size_t errlen )
{
	return db_from_pack( sc, pack, first, count, true, out, err, errlen );
}

extern "C" int rma_db_create_packed_async( rma_scanner_t *sc, const rma_pack_t *pack, int32_t first, int32_t count,
	rma_db_t **out, char *err, size_t errlen )
{
	return db_from_pack( sc, pack, first, count, false, out, err, errlen );
}

extern "C" int rma_db_create_packed_ranges( rma_scanner_t *sc, const rma_pack_t *pack, const int32_t *entry,
	const int32_t *pos_lo, const int32_t *pos_hi, int32_t n, rma_db_t **out, char *err, size_t errlen )
{
	*out = nullptr;
	const rma::PackFile	&pf = *rma_pack_file( pack );
	// the chosen entries side by side, each copied from where it lies in the pack (every entry starts
	// on a 32-base boundary: whole words); entries that follow each other in the pack go as one run
	std::vector<Piece>	pieces;
	std::vector<int64_t>	rel( size_t( std::max( n, 0 ) ) );
	std::vector<int32_t>	slen( size_t( std::max( n, 0 ) ) );
	int64_t	at = 0;		// mask words so far
	for( int i = 0; i < n; i++ ){
		const int	e = entry[ i ];
		if( e < 0 || e >= pf.count() ){
			snprintf( err, errlen, "entry %d is outside the packed database (%d entries)", e, pf.count() );
			return 1;
		}
		const int64_t	w1 = pf.base_off[ e ] / 32, nw1 = ( int64_t( pf.slen[ e ] ) + 31 ) / 32;
		rel[ i ] = at * 32;
		slen[ i ] = pf.slen[ e ];
		if( !pieces.empty() && pieces.back().amask + pieces.back().mask_words == pf.amask.data() + w1 )
			pieces.back().mask_words += size_t( nw1 );
		else if( nw1 > 0 )
			pieces.push_back( Piece{ pf.codes.data() + 2 * w1, pf.amask.data() + w1, size_t( nw1 ) } );
		at += nw1;
	}
	if( db_upload( device_of( sc ), pieces, rel.data(), slen.data(), n, pos_lo, pos_hi, true, out, err, errlen ) )
		return 1;
	return tile_at_creation( sc, out, err, errlen );
}

// ---------------------------------------------------------------- databases from device memory
// A pointer a kernel (or a copy on the device) is to be handed: memory of `device` the runtime knows, and
// bytes [lo, hi) from it inside its allocation where the runtime can say where that ends (memory it maps
// itself it cannot -- torch's expandable segments: the caller's extent governs alone).  A host pointer
// handed to a kernel faults the GPU; nothing is launched before this has said yes.
int rma::check_device_bytes( const void *p, int device, int64_t lo, int64_t hi, const char *what, char *err, size_t errlen )
{
	hipPointerAttribute_t	a;
	memset( &a, 0, sizeof( a ) );
	hipError_t	e = hipPointerGetAttributes( &a, p );
	if( e != hipSuccess ){
		( void )hipGetLastError();
		snprintf( err, errlen, "%s (%p) is not device memory: the HIP runtime does not know it (%s)", what, p, hipGetErrorString( e ) );
		return 1;
	}
	if( a.type != hipMemoryTypeDevice || a.isManaged ){
		const char	*kind = a.isManaged || a.type == hipMemoryTypeManaged ? "managed" : a.type == hipMemoryTypeHost ? "page-locked host" :
			a.type == hipMemoryTypeUnregistered ? "unregistered host" : "not device";
		snprintf( err, errlen, "%s (%p) is %s memory: device memory of device %d is needed", what, p, kind, device );
		return 1;
	}
	if( a.device != device ){
		snprintf( err, errlen, "%s (%p) is memory of device %d, the scanner is on device %d", what, p, a.device, device );
		return 1;
	}
	hipDeviceptr_t	base = nullptr;
	size_t	size = 0;
	e = hipMemGetAddressRange( &base, &size, const_cast<void *>( p ) );
	if( e != hipSuccess || base == nullptr ){
		( void )hipGetLastError();
		return 0;
	}
	const uintptr_t	q = reinterpret_cast<uintptr_t>( p ), b = reinterpret_cast<uintptr_t>( base );
	if( int64_t( q - b ) + lo < 0 || int64_t( q - b ) + hi > int64_t( size ) ){
		snprintf( err, errlen, "%s: bytes [%lld, %lld) from %p lie outside its allocation (%zu bytes at %p)", what,
			( long long )lo, ( long long )hi, p, size, base );
		return 1;
	}
	return 0;
}

// the caller's stream has reached this point before anything later on `on` runs
int rma::stream_after( hipStream_t on, hipStream_t caller, char *err, size_t errlen )
{
	hipError_t	e;
	{
		rma::Event	ev;		// (destroyed once the wait is queued: the wait holds what it needs)
		HIPCHK( ev.create( hipEventDisableTiming ) );
		e = hipEventRecord( ev.get(), caller );
		if( e == hipSuccess )
			e = hipStreamWaitEvent( on, ev.get(), 0 );
	}
	if( e != hipSuccess ){
		snprintf( err, errlen, "ordering behind the caller's stream: %s", hipGetErrorString( e ) );
		return 1;
	}
	return 0;
}

static int db_from_device_text( rma_scanner_t *sc, const void *text, int64_t text_bytes, int64_t lo, int64_t hi, const int64_t *start,
	const int32_t *slen, const int32_t *pos_lo, const int32_t *pos_hi, int32_t n, const uint8_t *table, const std::vector<uint8_t> &tab,
	bool default_table, void *stream, rma_db_t **out, char *err, size_t errlen );

extern "C" int rma_db_create_device( rma_scanner_t *sc, const void *text, int64_t text_bytes, const int64_t *start, const int32_t *slen,
	const int32_t *pos_lo, const int32_t *pos_hi, int32_t n, const uint8_t *table, void *stream, rma_db_t **out, char *err, size_t errlen )
{
	*out = nullptr;
	const int	device = device_of( sc );
	if( n < 0 || text_bytes < 0 || ( n > 0 && ( start == nullptr || slen == nullptr ) ) || ( pos_lo == nullptr ) != ( pos_hi == nullptr ) ){
		snprintf( err, errlen, "rma_db_create_device: %d entries, %lld bytes of text: bad arguments", n, ( long long )text_bytes );
		return 1;
	}
	// every entry inside the declared text, before anything else
	int64_t	lo = text_bytes, hi = 0;
	for( int i = 0; i < n; i++ ){
		if( slen[ i ] < 0 || start[ i ] < 0 ){
			snprintf( err, errlen, "entry %d: negative %s (start %lld, length %d)", i, slen[ i ] < 0 ? "length" : "start",
				( long long )start[ i ], slen[ i ] );
			return 1;
		}
		if( start[ i ] > text_bytes - slen[ i ] ){
			snprintf( err, errlen, "entry %d: bytes [%lld, %lld) lie past the text's %lld bytes", i, ( long long )start[ i ],
				( long long )start[ i ] + slen[ i ], ( long long )text_bytes );
			return 1;
		}
		if( slen[ i ] > 0 ){
			lo = std::min( lo, start[ i ] );
			hi = std::max( hi, start[ i ] + slen[ i ] );
		}
	}
	HIPCHK( hipSetDevice( device ) );
	if( hi > lo && rma::check_device_bytes( text, device, lo, hi, "the text", err, errlen ) )
		return 1;
	// the table: on the device (copied there, device to device) or on the host (checked, copied up)
	bool	table_on_device = false;
	std::vector<uint8_t>	tab( rma::letter_codes(), rma::letter_codes() + 256 );
	if( table != nullptr ){
		hipPointerAttribute_t	a;
		memset( &a, 0, sizeof( a ) );
		if( hipPointerGetAttributes( &a, table ) != hipSuccess )
			( void )hipGetLastError();
		else if( a.type == hipMemoryTypeDevice && !a.isManaged )
			table_on_device = true;
		if( table_on_device ){
			if( rma::check_device_bytes( table, device, 0, 256, "the table", err, errlen ) )
				return 1;
		}else{
			for( int c = 0; c < 256; c++ )
				if( table[ c ] > 4 ){
					snprintf( err, errlen, "table[ %d ] = %d: the codes are 0-3 and 4 (ambiguous)", c, table[ c ] );
					return 1;
				}
			tab.assign( table, table + 256 );
		}
	}
	return db_from_device_text( sc, text, text_bytes, lo, hi, start, slen, pos_lo, pos_hi, n, table_on_device ? table : nullptr, tab,
		table == nullptr, stream, out, err, errlen );
}

// rma_db_create_device() after its checks: the entries' words packed from text (bytes [lo, hi) of it hold them) behind
// the caller's stream, the tiling, the registration for rma_replay_device().  d_table: a table on the device, else tab.
static int db_from_device_text( rma_scanner_t *sc, const void *text, int64_t text_bytes, int64_t lo, int64_t hi, const int64_t *start,
	const int32_t *slen, const int32_t *pos_lo, const int32_t *pos_hi, int32_t n, const uint8_t *table, const std::vector<uint8_t> &tab,
	bool default_table, void *stream, rma_db_t **out, char *err, size_t errlen )
{
	const int	device = device_of( sc );
	const bool	table_on_device = table != nullptr;
	// the layout PackedDb::add() makes: every entry on a 32-base boundary, one after the other
	std::vector<int64_t>	base_off( static_cast<size_t>( n ) );
	int64_t	padded = 0;
	for( int i = 0; i < n; i++ ){
		base_off[ size_t( i ) ] = padded;
		padded += ( int64_t( slen[ i ] ) + 31 ) / 32 * 32;
	}
	const size_t	n_mask = size_t( padded / 32 );
	char	*extra = nullptr;
	if( db_alloc( device, base_off.data(), slen, n, pos_lo, pos_hi, n_mask, align256( size_t( std::max( n, 1 ) ) * 8 ) + 256, out, &extra, err, errlen ) )
		return 1;
	DbPtr	guard( *out, rma_db_destroy );
	rma_db	*db = guard.get();
	*out = nullptr;
	int64_t	*d_start = reinterpret_cast<int64_t *>( extra );
	uint8_t	*d_table = reinterpret_cast<uint8_t *>( extra + align256( size_t( std::max( n, 1 ) ) * 8 ) );
	hipStream_t	up = db->ctx->upload.get();
	// (host copies the database keeps until it is destroyed: the copies read them after this returns)
	db->h_text_start.assign( start, start + n );
	db->h_table = tab;
	db->text = static_cast<const uint8_t *>( text );
	db->text_bytes = text_bytes;
	db->text_lo = lo;
	db->text_hi = hi;
	db->d_text_start = d_start;
	db->d_table = d_table;
	db->default_table = default_table;
	if( n > 0 )
		HIPCHK( hipMemcpyAsync( d_start, db->h_text_start.data(), size_t( n ) * 8, hipMemcpyHostToDevice, up ) );
	if( !table_on_device )
		HIPCHK( hipMemcpyAsync( d_table, db->h_table.data(), 256, hipMemcpyHostToDevice, up ) );
	// the text (and a device table) as the caller's stream leaves them
	if( rma::stream_after( up, static_cast<hipStream_t>( stream ), err, errlen ) )
		return 1;
	if( table_on_device )
		HIPCHK( hipMemcpyAsync( d_table, table, 256, hipMemcpyDeviceToDevice, up ) );
	HIPCHK( rma::pack_text( static_cast<const uint8_t *>( text ), d_start, db->d_base_off, db->d_slen, n, int64_t( n_mask ), d_table,
		db->d_codes, db->d_amask, up ) );
	*out = guard.release();
	if( db_ready( out, false, err, errlen ) )
		return 1;
	if( tile_at_creation( sc, out, err, errlen ) )
		return 1;
	std::lock_guard<std::mutex>	lk( g_device_dbs_mu );
	g_device_dbs.insert( *out );
	return 0;
}

// ---------------------------------------------------------------- databases from FASTA text in device memory
// The entries and their letters are found on the device (rm_fasta_dev.hip): summaries of the chunks, a scan of them,
// then the letters into a clean text the database owns.  Two synchronisations of the upload stream teach the host
// what it cannot go on without -- the totals (to allocate), then the entries' offsets and definition lines (to name
// the entries and to refuse what the readers have a diagnostic for).  From there on the database is
// db_from_device_text()'s over the clean text.
extern "C" int rma_db_create_device_fasta( rma_scanner_t *sc, const void *text, int64_t text_bytes, int32_t maxslen, void *stream,
	rma_db_t **out, char *err, size_t errlen )
{
	*out = nullptr;
	const int	device = device_of( sc );
	if( text_bytes < 0 || maxslen < 0 || ( text_bytes > 0 && text == nullptr ) ){
		snprintf( err, errlen, "rma_db_create_device_fasta: %lld bytes of text, maxslen %d: bad arguments", ( long long )text_bytes, maxslen );
		return 1;
	}
	const int64_t	lim = maxslen > 0 ? int64_t( maxslen ) + 1 : 30000000 + 1;	// as rma_pack_read: -N n reads n letters
	HIPCHK( hipSetDevice( device ) );
	if( text_bytes > 0 && rma::check_device_bytes( text, device, 0, text_bytes, "the text", err, errlen ) )
		return 1;
	DevCtx	*ctx = dev_ctx( device, err, errlen );
	if( ctx == nullptr )
		return 1;
	hipStream_t	up = ctx->upload.get();
	const std::vector<uint8_t>	tab( rma::letter_codes(), rma::letter_codes() + 256 );
	// device blocks of this call: back to the cache on every way out, once the upload stream is done with them; the
	// clean text goes to the database instead
	struct Blocks {
		DevCtx	*ctx;
		Block	work, entries, headers, clean;
		bool	idle = false;		// nothing on the upload stream uses them any more
		~Blocks()
		{
			if( !idle )
				( void )hipStreamSynchronize( ctx->upload.get() );
			ctx->give( work ); ctx->give( entries ); ctx->give( headers ); ctx->give( clean );
		}
	}	b{ ctx, {}, {}, {}, {} };
	const uint8_t	*t8 = static_cast<const uint8_t *>( text );
	rma::FdPrefix	totals{ 0, 0, 0, 0 };
	const rma::FdSummary	*d_local = nullptr;
	const rma::FdPrefix	*d_block_pre = nullptr, *d_totals = nullptr;
	if( text_bytes > 0 ){
		const int64_t	chunks = rma::fasta_chunks( text, text_bytes ), blocks = rma::fasta_blocks( chunks );
		if( chunks > 0x7fffffffll ){
			snprintf( err, errlen, "rma_db_create_device_fasta: %lld bytes of text are more than 2^31 chunks", ( long long )text_bytes );
			return 1;
		}
		const size_t	o_sum = 0, o_local = o_sum + align256( size_t( chunks ) * sizeof( rma::FdSummary ) );
		const size_t	o_bsum = o_local + align256( size_t( chunks ) * sizeof( rma::FdSummary ) );
		const size_t	o_bpre = o_bsum + align256( size_t( blocks ) * sizeof( rma::FdSummary ) );
		const size_t	o_tot = o_bpre + align256( size_t( blocks ) * sizeof( rma::FdPrefix ) );
		HIPCHK( ctx->take( o_tot + 256, &b.work ) );
		char	*w = static_cast<char *>( b.work.p );
		d_local = reinterpret_cast<rma::FdSummary *>( w + o_local );
		d_block_pre = reinterpret_cast<rma::FdPrefix *>( w + o_bpre );
		d_totals = reinterpret_cast<rma::FdPrefix *>( w + o_tot );
		// the text as the caller's stream leaves it
		if( rma::stream_after( up, static_cast<hipStream_t>( stream ), err, errlen ) )
			return 1;
		HIPCHK( rma::fasta_index( t8, text_bytes, reinterpret_cast<rma::FdSummary *>( w + o_sum ), reinterpret_cast<rma::FdSummary *>( w + o_local ),
			reinterpret_cast<rma::FdSummary *>( w + o_bsum ), reinterpret_cast<rma::FdPrefix *>( w + o_bpre ),
			reinterpret_cast<rma::FdPrefix *>( w + o_tot ), up ) );
		unsigned char	first_byte = 0;
		HIPCHK( hipMemcpyAsync( &totals, d_totals, sizeof( totals ), hipMemcpyDeviceToHost, up ) );
		HIPCHK( hipMemcpyAsync( &first_byte, t8, 1, hipMemcpyDeviceToHost, up ) );
		HIPCHK( hipStreamSynchronize( up ) );
		if( first_byte != '>' ){
			snprintf( err, errlen, "entry 0 at byte 0: the text does not begin with '>'" );
			return 1;
		}
		if( totals.starts > 0x7fffffffll ){
			snprintf( err, errlen, "the text holds %lld entries: more than a database's %d", ( long long )totals.starts, 0x7fffffff );
			return 1;
		}
	}
	const int32_t	n = int32_t( totals.starts );
	const size_t	nn = size_t( n );
	std::vector<int64_t>	gt_off( nn ), def_end( nn ), first( nn );
	std::vector<int32_t>	slen( nn );
	std::vector<std::string>	sids( nn ), sdefs( nn );
	if( n > 0 ){
		HIPCHK( ctx->take( size_t( std::max<int64_t>( totals.letters, 1 ) ), &b.clean ) );
		const size_t	o_end = align256( nn * 8 ), o_first = 2 * o_end;
		HIPCHK( ctx->take( 3 * o_end, &b.entries ) );
		char	*e = static_cast<char *>( b.entries.p );
		int64_t	*d_gt = reinterpret_cast<int64_t *>( e ), *d_end = reinterpret_cast<int64_t *>( e + o_end );
		int64_t	*d_first = reinterpret_cast<int64_t *>( e + o_first );
		HIPCHK( rma::fasta_apply( t8, text_bytes, d_local, d_block_pre, d_totals, static_cast<uint8_t *>( b.clean.p ), d_gt, d_end, d_first, up ) );
		HIPCHK( hipMemcpyAsync( gt_off.data(), d_gt, nn * 8, hipMemcpyDeviceToHost, up ) );
		HIPCHK( hipMemcpyAsync( def_end.data(), d_end, nn * 8, hipMemcpyDeviceToHost, up ) );
		HIPCHK( hipMemcpyAsync( first.data(), d_first, nn * 8, hipMemcpyDeviceToHost, up ) );
		HIPCHK( hipStreamSynchronize( up ) );
		// the definition lines, one after the other, each capped (a longer one is refused below without its bytes)
		std::vector<int64_t>	hdr_off( nn + 1 );
		hdr_off[ 0 ] = 0;
		for( size_t i = 0; i < nn; i++ ){
			if( gt_off[ i ] < 0 || def_end[ i ] <= gt_off[ i ] || def_end[ i ] > text_bytes || first[ i ] < 0 || first[ i ] > totals.letters ||
				( i > 0 && ( gt_off[ i ] <= gt_off[ i - 1 ] || first[ i ] < first[ i - 1 ] ) ) ){
				snprintf( err, errlen, "entry %zu: the text changed while it was being read", i );
				return 1;
			}
			hdr_off[ i + 1 ] = hdr_off[ i ] + std::min<int64_t>( def_end[ i ] - gt_off[ i ], rma::FD_HEADER_CAP );
		}
		HIPCHK( ctx->take( size_t( hdr_off[ nn ] ), &b.headers ) );
		// (the entries' first letters are on the host by now: their array takes the header offsets)
		HIPCHK( hipMemcpyAsync( d_first, hdr_off.data(), nn * 8, hipMemcpyHostToDevice, up ) );
		HIPCHK( rma::fasta_headers( t8, text_bytes, d_gt, d_end, d_first, n, static_cast<uint8_t *>( b.headers.p ), up ) );
		std::vector<char>	hdr( size_t( hdr_off[ nn ] ) );
		HIPCHK( hipMemcpyAsync( hdr.data(), b.headers.p, hdr.size(), hipMemcpyDeviceToHost, up ) );
		HIPCHK( hipStreamSynchronize( up ) );
		// names and refusals, entry by entry in the text's order: FastaStream::parse's verdicts
		for( size_t i = 0; i < nn; i++ ){
			const char	*h = hdr.data() + hdr_off[ i ], *rest = nullptr;
			const int64_t	line = def_end[ i ] - gt_off[ i ], letters = ( i + 1 < nn ? first[ i + 1 ] : totals.letters ) - first[ i ];
			int	why = line > rma::FD_HEADER_CAP ? int( rma::DEFLINE_LONG ) :
				rma::parse_defline( h, h + ( hdr_off[ i + 1 ] - hdr_off[ i ] ), sids[ i ], sdefs[ i ], &rest );
			const char	*reason = why == rma::DEFLINE_NOT_GT ? "does not begin with '>'" : why == rma::DEFLINE_UNNAMED ? "unnamed entry" :
				why == rma::DEFLINE_LONG ? "definition line too long (19999 bytes or more)" :
				why == rma::DEFLINE_NUL ? "NUL in the definition line" : nullptr;
			if( reason == nullptr && letters >= lim )
				reason = "sequence too long";
			if( reason != nullptr ){
				if( why == rma::DEFLINE_LONG )
					snprintf( err, errlen, "entry %zu at byte %lld: %s: a line of %lld bytes", i, ( long long )gt_off[ i ], reason, ( long long )line );
				else if( why == rma::DEFLINE_OK )
					snprintf( err, errlen, "entry %zu at byte %lld: %s: %lld letters, the limit is %lld", i, ( long long )gt_off[ i ], reason,
						( long long )letters, ( long long )lim - 1 );
				else
					snprintf( err, errlen, "entry %zu at byte %lld: %s", i, ( long long )gt_off[ i ], reason );
				return 1;
			}
			slen[ i ] = int32_t( letters );
			sids[ i ].resize( strlen( sids[ i ].c_str() ) );	// (as the readers deliver it: a C string)
		}
	}
	if( db_from_device_text( sc, b.clean.p, totals.letters, 0, totals.letters, first.data(), slen.data(), nullptr, nullptr, n, nullptr, tab, true,
		stream, out, err, errlen ) )
		return 1;
	b.idle = true;
	// (the pack kernel follows the apply kernel on the upload stream; the caller's text is not read again)
	( *out )->text_blk = b.clean;
	b.clean = Block{};
	( *out )->sids = std::move( sids );
	( *out )->sdefs = std::move( sdefs );
	return 0;
}

// ---------------------------------------------------------------- the text of a packed database, made on the device
// A database of packed words gets what rma_db_create_device_fasta()'s has: a text of its own in text_blk, one byte per
// base, made by the kernels of rm_dbtext_dev.hip from its words and the letters at its masked positions.  Everything
// is refused before anything of the database changes; the one wait is for the word of the check, behind the fill.
static int db_text_attach( const char *who, rma_db_t *db, const char *exc, const int64_t *exc_off, void *stream, char *err, size_t errlen )
{
	if( db == nullptr || !is_live_db( db ) ){
		snprintf( err, errlen, "%s: the database (%p) has been destroyed or was never made", who, static_cast<const void *>( db ) );
		return 1;
	}
	if( rma::is_device_db( db ) || db->text != nullptr ){
		snprintf( err, errlen, "%s: the database already has its text in device memory (made from a tensor, from FASTA text, or attached before)", who );
		return 1;
	}
	{
		std::lock_guard<std::mutex>	lk( db->mu );
		if( !db->busy.empty() ){
			snprintf( err, errlen, "%s: a scan of the database is in flight: end it first", who );
			return 1;
		}
	}
	const int32_t	n = db->n_seq;
	const size_t	nn = size_t( n );
	const int64_t	n_mask = db->padded_bases / 32;
	if( exc != nullptr ){
		if( exc_off == nullptr ){
			snprintf( err, errlen, "%s: exceptions without their offsets: bad arguments", who );
			return 1;
		}
		for( int32_t i = 0; i <= n; i++ )
			if( i == 0 ? exc_off[ 0 ] != 0 : exc_off[ i ] < exc_off[ i - 1 ] ){
				snprintf( err, errlen, "%s: exc_off[ %d ] = %lld: the offsets ascend from 0", who, i, ( long long )exc_off[ i ] );
				return 1;
			}
	}
	// the entries' words inside the arrays (every database made here has them so: the kernels read through these)
	std::vector<int64_t>	start( nn );
	int64_t	text_bytes = 0;
	for( size_t i = 0; i < nn; i++ ){
		const int64_t	b = db->h_base_off[ i ];
		if( b < 0 || b % 32 != 0 || db->h_slen[ i ] < 0 || b / 32 + ( int64_t( db->h_slen[ i ] ) + 31 ) / 32 > n_mask ){
			snprintf( err, errlen, "%s: entry %zu: bases [%lld, %lld) are not whole words of the database's %lld", who, i, ( long long )b,
				( long long )b + db->h_slen[ i ], ( long long )n_mask );
			return 1;
		}
		start[ i ] = text_bytes;
		text_bytes += rma::dbtext_entry_bytes( db->h_slen[ i ] );
	}
	const int64_t	n_exc = exc != nullptr ? exc_off[ n ] : 0;
	HIPCHK( hipSetDevice( db->device ) );
	DevCtx	*ctx = db->ctx;
	hipStream_t	up = ctx->upload.get();
	// the blocks of this call: back to the cache on every way out, once the upload stream is done with them; the text
	// goes to the database instead
	struct Blocks {
		DevCtx	*ctx;
		Block	work, text;
		bool	idle = true;		// nothing on the upload stream uses them
		~Blocks()
		{
			if( !idle )
				( void )hipStreamSynchronize( ctx->upload.get() );
			ctx->give( work ); ctx->give( text );
		}
	}	b{ ctx, {}, {} };
	rma::DbTextArgs	a;
	memset( &a, 0, sizeof( a ) );
	size_t	scan_tmp = 0;
	a.n_mask = n_mask;
	HIPCHK( rma::dbtext_directory( a, nullptr, &scan_tmp, up ) );
	// work: dir | exc_off | exc_base | bad | the scan's scratch | exc;  text: the text | text_start
	Carver	cw, ct;
	const size_t	runs = size_t( rma::dbtext_dir_runs( n_mask ) );
	cw.take<uint64_t>( nullptr, runs ); cw.take<int64_t>( nullptr, nn + 1 ); cw.take<int64_t>( nullptr, nn + 1 );
	cw.take<unsigned long long>( nullptr, 1 ); cw.take<char>( nullptr, scan_tmp + 1 ); cw.take<char>( nullptr, size_t( n_exc ) + 1 );
	ct.take<uint8_t>( nullptr, size_t( text_bytes ) + 1 ); ct.take<int64_t>( nullptr, nn + 1 );
	HIPCHK( ctx->take( cw.at, &b.work ) );
	HIPCHK( ctx->take( ct.at, &b.text ) );
	cw = Carver(); ct = Carver();
	a.dir = cw.take<uint64_t>( b.work.p, runs );
	int64_t	*d_exc_off = cw.take<int64_t>( b.work.p, nn + 1 );
	a.exc_base = cw.take<int64_t>( b.work.p, nn + 1 );
	a.bad = cw.take<unsigned long long>( b.work.p, 1 );
	void	*d_scan_tmp = cw.take<char>( b.work.p, scan_tmp + 1 );
	char	*d_exc = cw.take<char>( b.work.p, size_t( n_exc ) + 1 );
	a.text = ct.take<uint8_t>( b.text.p, size_t( text_bytes ) + 1 );
	int64_t	*d_start = ct.take<int64_t>( b.text.p, nn + 1 );
	a.codes = db->d_codes;
	a.amask = db->d_amask;
	a.base_off = db->d_base_off;
	a.slen = db->d_slen;
	a.n = n;
	a.exc = exc != nullptr ? d_exc : nullptr;
	a.exc_off = exc != nullptr ? d_exc_off : nullptr;
	a.n_exc = n_exc;
	a.text_start = d_start;
	a.text_bytes = text_bytes;
	rma::Event	t0, t1;
	HIPCHK( t0.create( hipEventDefault ) );
	HIPCHK( t1.create( hipEventDefault ) );
	unsigned long long	bad = rma::DT_BAD_NONE;
	// behind the caller's stream and the database's words
	if( rma::stream_after( up, static_cast<hipStream_t>( stream ), err, errlen ) )
		return 1;
	HIPCHK( hipStreamWaitEvent( up, db->ready.get(), 0 ) );
	b.idle = false;
	if( n > 0 )
		HIPCHK( hipMemcpyAsync( d_start, start.data(), nn * 8, hipMemcpyHostToDevice, up ) );
	if( exc != nullptr ){
		HIPCHK( hipMemcpyAsync( d_exc_off, exc_off, ( nn + 1 ) * 8, hipMemcpyHostToDevice, up ) );
		if( n_exc > 0 )
			HIPCHK( hipMemcpyAsync( d_exc, exc, size_t( n_exc ), hipMemcpyHostToDevice, up ) );
	}
	HIPCHK( hipMemsetAsync( a.bad, 0xff, sizeof( unsigned long long ), up ) );
	HIPCHK( rma::dbtext_directory( a, d_scan_tmp, &scan_tmp, up ) );
	HIPCHK( rma::dbtext_check( a, up ) );
	HIPCHK( hipEventRecord( t0.get(), up ) );
	HIPCHK( rma::dbtext_fill( a, up ) );
	HIPCHK( hipEventRecord( t1.get(), up ) );
	HIPCHK( hipMemcpyAsync( &bad, a.bad, sizeof( bad ), hipMemcpyDeviceToHost, up ) );
	HIPCHK( hipStreamSynchronize( up ) );
	b.idle = true;
	if( bad != rma::DT_BAD_NONE ){
		const int32_t	e = rma::dbtext_bad_entry( bad );
		const int64_t	have = exc_off[ e + 1 ] - exc_off[ e ];
		if( rma::dbtext_bad_kind( bad ) == rma::DT_BAD_COUNT )
			snprintf( err, errlen, "%s: entry %d: its mask has %u bases set, its exceptions are %lld", who, e, rma::dbtext_bad_value( bad ), ( long long )have );
		else{
			int64_t	k = 0;
			while( k + 1 < have && rma::dbtext_exc_letter( static_cast<unsigned char>( exc[ exc_off[ e ] + k ] ) ) )
				k++;
			snprintf( err, errlen, "%s: entry %d: exception %lld is byte 0x%02x: a lower-case letter other than a, c, g and t stands at a masked position",
				who, e, ( long long )k, static_cast<unsigned char>( exc[ exc_off[ e ] + k ] ) );
		}
		return 1;
	}
	float	ms = -1.0f;
	if( hipEventElapsedTime( &ms, t0.get(), t1.get() ) != hipSuccess ){
		( void )hipGetLastError();
		ms = -1.0f;
	}
	// from here on it is a rma_db_create_device() database of the readers' letters over its own text
	int64_t	lo = text_bytes, hi = 0;
	for( size_t i = 0; i < nn; i++ )
		if( db->h_slen[ i ] > 0 ){
			lo = std::min( lo, start[ i ] );
			hi = std::max( hi, start[ i ] + db->h_slen[ i ] );
		}
	HIPCHK( hipEventRecord( db->ready.get(), up ) );
	db->h_text_start = std::move( start );
	db->text = a.text;
	db->text_bytes = text_bytes;
	db->text_lo = lo;
	db->text_hi = hi;
	db->d_text_start = d_start;
	db->default_table = true;
	db->text_fill_ms = ms;
	db->text_blk = b.text;
	b.text = Block{};
	std::lock_guard<std::mutex>	lk( g_device_dbs_mu );
	g_device_dbs.insert( db );
	return 0;
}

extern "C" int rma_db_text_attach( rma_db_t *db, const char *exc, const int64_t *exc_off, void *stream, char *err, size_t errlen )
{
	return db_text_attach( "rma_db_text_attach", db, exc, exc_off, stream, err, errlen );
}

extern "C" int rma_db_text_attach_pack( rma_db_t *db, const rma_pack_t *pk, const int32_t *entry, int32_t first, void *stream,
	char *err, size_t errlen )
{
	const char	*who = "rma_db_text_attach_pack";
	if( db == nullptr || !is_live_db( db ) ){
		snprintf( err, errlen, "%s: the database (%p) has been destroyed or was never made", who, static_cast<const void *>( db ) );
		return 1;
	}
	const rma::PackFile	&pf = *rma_pack_file( pk );
	const int32_t	n = db->n_seq;
	// the exceptions of the named entries, one after the other
	std::vector<char>	exc;
	std::vector<int64_t>	exc_off( size_t( n ) + 1, 0 );
	std::vector<std::string>	sids( static_cast<size_t>( n ) ), sdefs( static_cast<size_t>( n ) );
	for( int32_t i = 0; i < n; i++ ){
		const int64_t	e = entry != nullptr ? int64_t( entry[ i ] ) : int64_t( first ) + i;
		if( e < 0 || e >= pf.count() ){
			snprintf( err, errlen, "%s: entry %d of the database is entry %lld of the pack, which has %d entries", who, i, ( long long )e, pf.count() );
			return 1;
		}
		if( pf.slen[ size_t( e ) ] != db->h_slen[ size_t( i ) ] ){
			snprintf( err, errlen, "%s: entry %d of the database has %d bases, entry %lld of the pack %d", who, i, db->h_slen[ size_t( i ) ],
				( long long )e, pf.slen[ size_t( e ) ] );
			return 1;
		}
		const int64_t	x0 = pf.exc_off[ size_t( e ) ], x1 = e + 1 < pf.count() ? pf.exc_off[ size_t( e ) + 1 ] : int64_t( pf.exc.size() );
		if( x0 < 0 || x1 < x0 || x1 > int64_t( pf.exc.size() ) ){
			snprintf( err, errlen, "%s: entry %lld of the pack: exceptions [%lld, %lld) of %zu", who, ( long long )e, ( long long )x0, ( long long )x1, pf.exc.size() );
			return 1;
		}
		exc.insert( exc.end(), pf.exc.begin() + x0, pf.exc.begin() + x1 );
		exc_off[ size_t( i ) + 1 ] = int64_t( exc.size() );
		sids[ size_t( i ) ] = pf.sid( int( e ) );
		sdefs[ size_t( i ) ] = pf.sdef( int( e ) );
	}
	exc.push_back( 0 );		// (never null: a pack without exceptions still has its counts checked)
	if( db_text_attach( who, db, exc.data(), exc_off.data(), stream, err, errlen ) )
		return 1;
	db->sids = std::move( sids );
	db->sdefs = std::move( sdefs );
	return 0;
}

extern "C" int rma_db_read_text( const rma_db_t *db, int32_t i, char *buf, char *err, size_t errlen )
{
	if( db == nullptr || !rma::is_device_db( db ) ){
		snprintf( err, errlen, "rma_db_read_text: the database (%p) has no text in device memory or has been destroyed", static_cast<const void *>( db ) );
		return 1;
	}
	if( i < 0 || i >= db->n_seq ){
		snprintf( err, errlen, "rma_db_read_text: entry %d of %d", i, db->n_seq );
		return 1;
	}
	HIPCHK( hipSetDevice( db->device ) );
	HIPCHK( hipEventSynchronize( db->ready.get() ) );
	if( db->h_slen[ size_t( i ) ] > 0 )
		HIPCHK( hipMemcpy( buf, db->text + db->h_text_start[ size_t( i ) ], size_t( db->h_slen[ size_t( i ) ] ), hipMemcpyDeviceToHost ) );
	return 0;
}

extern "C" float rma_db_text_fill_ms( const rma_db_t *db ) { return db != nullptr ? db->text_fill_ms : -1.0f; }

extern "C" int32_t rma_db_entries( const rma_db_t *db ) { return db->n_seq; }

extern "C" void rma_fasta_device_shape( int32_t shape[ 3 ] )
{
	shape[ 0 ] = rma::FD_CHUNK;
	shape[ 1 ] = rma::FD_SCAN_BLOCK;
	shape[ 2 ] = rma::FD_HEADER_CAP;
}

extern "C" int rma_db_entry_name( const rma_db_t *db, int32_t i, const char **sid, const char **sdef )
{
	if( db == nullptr || i < 0 || size_t( i ) >= db->sids.size() )
		return 1;
	if( sid != nullptr )
		*sid = db->sids[ size_t( i ) ].c_str();
	if( sdef != nullptr )
		*sdef = db->sdefs[ size_t( i ) ].c_str();
	return 0;
}

extern "C" int64_t rma_db_mask_words( const rma_db_t *db ) { return db->padded_bases / 32; }

extern "C" int rma_db_read_packed( const rma_db_t *db, uint32_t *codes, uint32_t *amask, int64_t *base_off, int32_t *slen,
	char *err, size_t errlen )
{
	HIPCHK( hipSetDevice( db->device ) );
	HIPCHK( hipEventSynchronize( db->ready.get() ) );
	const size_t	n_mask = size_t( db->padded_bases / 32 ), n = size_t( db->n_seq );
	if( codes != nullptr && n_mask > 0 )
		HIPCHK( hipMemcpy( codes, db->d_codes, n_mask * 8, hipMemcpyDeviceToHost ) );
	if( amask != nullptr && n_mask > 0 )
		HIPCHK( hipMemcpy( amask, db->d_amask, n_mask * 4, hipMemcpyDeviceToHost ) );
	if( base_off != nullptr && n > 0 )
		HIPCHK( hipMemcpy( base_off, db->d_base_off, n * 8, hipMemcpyDeviceToHost ) );
	if( slen != nullptr && n > 0 )
		HIPCHK( hipMemcpy( slen, db->d_slen, n * 4, hipMemcpyDeviceToHost ) );
	return 0;
}

extern "C" void rma_letter_codes( uint8_t codes[ 256 ] ) { memcpy( codes, rma::letter_codes(), 256 ); }

extern "C" int rma_db_wait( rma_db_t *db, char *err, size_t errlen )
{
	HIPCHK( hipSetDevice( db->device ) );
	HIPCHK( hipEventSynchronize( db->ready.get() ) );
	return 0;
}

extern "C" void rma_db_destroy( rma_db_t *db )
{
	if( db == nullptr )
		return;
	{
		std::lock_guard<std::mutex>	lk( g_device_dbs_mu );
		g_device_dbs.erase( db );
		g_live_dbs.erase( db );
	}
	( void )hipSetDevice( db->device );
	// scans of this database that were begun and not ended: their kernels read it
	std::vector<rma_scanner *>	busy;
	{
		std::lock_guard<std::mutex>	lk( db->mu );
		busy = db->busy;
	}
	for( rma_scanner *sc : busy )
		( void )hipStreamSynchronize( sc->stream.get() );
	if( db->ready.get() != nullptr )
		( void )hipEventSynchronize( db->ready.get() );	// (an upload still on its way into the block)
	// (a tiling's two copies may still be on their way -- made by rma_db_attach() on a scanner's stream, or behind the
	// words on the upload stream after db->ready was recorded: they read the layout's host vectors and write its block)
	for( auto &l : db->layouts )
		if( l->ready.get() != nullptr )
			( void )hipEventSynchronize( l->ready.get() );
	if( db->ctx != nullptr ){
		db->ctx->give( db->blk );
		db->ctx->give( db->text_blk );
		for( auto &l : db->layouts )
			db->ctx->give( l->blk );
	}
	delete db;
}

extern "C" int64_t rma_db_bases( const rma_db_t *db ) { return db->total_bases; }

// ---------------------------------------------------------------- pinned host memory
// A packed database in memory whose words are page-locked uploads by DMA, without a staging copy,
// and asynchronously (rma_db_create_packed_async).  Locking costs about as much as one upload, so it
// pays for a pack that is uploaded more than once or under a running scan.
extern "C" int rma_pack_pin( rma_pack_t *pack, char *err, size_t errlen )
{
	rma::PackFile	&pf = *const_cast<rma::PackFile *>( rma_pack_file( pack ) );
	if( pf.pin.unreg != nullptr )
		return 0;
	void	*c = pf.codes.empty() ? nullptr : pf.codes.data(), *m = pf.amask.empty() ? nullptr : pf.amask.data();
	if( c != nullptr )
		HIPCHK( hipHostRegister( c, pf.codes.size() * 4, hipHostRegisterDefault ) );
	if( m != nullptr ){
		hipError_t	e = hipHostRegister( m, pf.amask.size() * 4, hipHostRegisterDefault );
		if( e != hipSuccess ){
			if( c != nullptr )
				( void )hipHostUnregister( c );
			snprintf( err, errlen, "hipHostRegister: %s", hipGetErrorString( e ) );
			return 1;
		}
	}
	pf.pin.c = c;
	pf.pin.m = m;
	pf.pin.unreg = []( void *p ){ ( void )hipHostUnregister( p ); };
	return 0;
}

// ---------------------------------------------------------------- tilings
// The tiling of database db for scanner sc's launch shape (rma::choose_layout): made and uploaded when the
// scanner first meets the database with that shape, found again afterwards.
static const Layout *layout_for( rma_scanner_t *sc, const rma_db_t *cdb, char *err, size_t errlen, hipStream_t on )
{
	if( on == nullptr )
		on = sc->stream.get();
	rma_db	*db = const_cast<rma_db *>( cdb );
	const rma::DbShape	shape{ db->n_seq, db->sum_slen, db->padded_bases, !db->h_pos_lo.empty(), db->ascending };
	const rma::LayoutKey	key = rma::choose_layout( sc->plan, sc->opt, shape, sc->grid_blocks / 8 );
	std::lock_guard<std::mutex>	lk( db->mu );
	for( auto &l : db->layouts )
		if( static_cast<const rma::LayoutKey &>( *l ) == key )
			return l.get();
	std::unique_ptr<Layout>	l( new Layout );
	static_cast<rma::LayoutKey &>( *l ) = key;
	rma::make_tiling( key, db->h_slen, db->h_base_off, db->h_pos_lo, db->h_pos_hi, db->padded_bases, l.get() );
	const std::vector<int64_t>	&tile_start = l->h_tile_start;
	const std::vector<int32_t>	&tile_seq = l->h_tile_seq, &tile_meta = l->h_tile_meta;
	const size_t	o_seq = align256( tile_start.size() * 8 ), o_meta = align256( o_seq + tile_seq.size() * 4 );
	hipError_t	e = db->ctx->take( o_meta + tile_meta.size() * 4, &l->blk );
	// On the stream given: the upload stream when the database is being made for a scanner (its first
	// scan then finds the tiling there), else the scanner's.  The host copies stay with the layout and
	// an event says when the copies are done, so nothing waits here.
	if( e == hipSuccess ){
		l->d_tile_start = static_cast<int64_t *>( l->blk.p );
		l->d_tile_seq = reinterpret_cast<int32_t *>( static_cast<char *>( l->blk.p ) + o_seq );
		e = hipMemcpyAsync( l->d_tile_start, tile_start.data(), tile_start.size() * 8, hipMemcpyHostToDevice, on );
	}
	if( e == hipSuccess )
		e = hipMemcpyAsync( l->d_tile_seq, tile_seq.data(), tile_seq.size() * 4, hipMemcpyHostToDevice, on );
	if( e == hipSuccess && !tile_meta.empty() ){
		l->d_tile_meta = reinterpret_cast<int32_t *>( static_cast<char *>( l->blk.p ) + o_meta );
		e = hipMemcpyAsync( l->d_tile_meta, tile_meta.data(), tile_meta.size() * 4, hipMemcpyHostToDevice, on );
	}
	if( e == hipSuccess )
		e = l->ready.create( hipEventDisableTiming );
	if( e == hipSuccess )
		e = hipEventRecord( l->ready.get(), on );
	if( e != hipSuccess ){
		db->ctx->give( l->blk );
		snprintf( err, errlen, "tiling of the database: %s", hipGetErrorString( e ) );
		return nullptr;
	}
	db->layouts.push_back( std::move( l ) );
	return db->layouts.back().get();
}

extern "C" int rma_db_attach( rma_scanner_t *sc, rma_db_t *db, char *err, size_t errlen )
{
	if( db->device != sc->device ){
		snprintf( err, errlen, "the database lives on device %d, the scanner on device %d", db->device, sc->device );
		return 1;
	}
	HIPCHK( hipSetDevice( sc->device ) );
	return layout_for( sc, db, err, errlen ) != nullptr ? 0 : 1;
}

static DbView view_of( const rma_db *db, const Layout *l )
{
	DbView	v;
	v.codes = db->d_codes;
	v.amask = db->d_amask;
	v.base_off = db->d_base_off;
	v.slen = db->d_slen;
	v.tile_start = l->d_tile_start;
	v.tile_seq = l->d_tile_seq;
	v.tile_meta = l->d_tile_meta;
	v.concat_bases = l->concat ? l->concat_bases : 0;
	v.pos_lo = db->d_pos_lo;
	v.pos_hi = db->d_pos_hi;
	v.n_seq = db->n_seq;
	v.strands = l->strands;
	v.tile_t = l->tile_t;
	v.n_tiles = l->n_tiles;
	return v;
}

// ---------------------------------------------------------------- scans
// Work areas that grow when a scan asks for more; what was there is freed first, and a failure leaves none.
// The spill area: room for `need` items a workgroup.
static int grow_spill( rma_scanner_t *sc, unsigned long long need, char *err, size_t errlen )
{
	HIPCHK( sc->d_spill.exact( size_t( sc->spill_blocks ) * ( size_t( need ) + 1024 ) * sizeof( unsigned ) ) );
	return 0;
}

// The pooled instance's d_pool: the drain kernel's list of `list` items, then `cap` items of every workgroup's pool.
static int grow_pool( rma_scanner_t *sc, int list, int cap, char *err, size_t errlen )
{
	sc->pool_cap = sc->glist_cap = 0;
	HIPCHK( sc->d_pool.exact( ( size_t( list ) + size_t( sc->grid_blocks ) * cap ) * RMK_POOL_WORDS * sizeof( unsigned ) ) );
	sc->pool_cap = cap;
	sc->glist_cap = list;
	return 0;
}

// The pinned staging buffer of the records (the copy back is a single DMA): twice `words` when they do not fit.
static int grow_h_raw( rma_scanner_t *sc, size_t words, char *err, size_t errlen )
{
	if( words > sc->h_raw_cap() )
		HIPCHK( sc->h_raw.exact( words * 2 * sizeof( int32_t ) ) );
	return 0;
}

// (tail: the caller enqueues the scan's tail behind the kernels and the counters' copy behind that, launch_tail)
static int launch_search( rma_scanner_t *sc, char *err, size_t errlen, bool tail = false )
{
	const rma_scanner::InFlight	&f = sc->fly;
	sc->search_launches++;
	HIPCHK( hipMemsetAsync( sc->counters(), 0, RMK_N_COUNTERS * sizeof( unsigned long long ), sc->stream.get() ) );
	rmk_search_args	a;
	a.d_prog = sc->d_prog.as<rmd_program_t>();
	a.prog_bytes = sc->prog_bytes;
	a.qcap = f.lay->qcap;
	a.db = view_of( f.db, f.lay );
	const bool	listed = f.plan.listed, drain = listed && sc->glist_cap > 0;
	a.hb = HitBuf{ sc->hits(), sc->counters() + RMK_C_COUNT, sc->counters() + RMK_C_TICKET, sc->hit_cap(), sc->d_spill.as<unsigned>(), sc->spill_cap(), sc->d_pool.as<unsigned>(), sc->pool_cap,
		sc->opt.pool_min, sc->opt.pool_refill, listed ? sc->glist_cap : 0 };
	a.tile_bytes = f.plan.tile_bytes;
	a.dbg = sc->opt.dbg | ( sc->whole_items ? RMK_DBG_WHOLE_ITEMS : 0 );
	HIPCHK( hipEventRecord( sc->ev[ 0 ].get(), sc->stream.get() ) );
	HIPCHK( rmk_launch_search( f.plan.inst, f.plan.grid, f.plan.lds, sc->stream.get(), a ) );
	sc->drained = drain;
	sc->last_launch[ 0 ] = f.plan.grid;
	sc->last_launch[ 1 ] = int( f.plan.lds );
	sc->last_launch[ 2 ] = drain ? f.plan.drain_grid : 0;
	sc->last_launch[ 3 ] = int( f.plan.beside );
	sc->searched = true;
	sc->efn_ran = false;
	if( drain ){	// the items the search kernel left in the list: walked by a kernel of their own
		HIPCHK( hipEventRecord( sc->ev[ 4 ].get(), sc->stream.get() ) );
		a.tile_bytes = f.plan.drain_nib;
		HIPCHK( rmk_launch_lean_drain( f.plan.drain_grid, f.plan.drain_lds, sc->stream.get(), a ) );
	}
	HIPCHK( hipEventRecord( sc->ev[ 1 ].get(), sc->stream.get() ) );
	// RMK_C_COUNT, RMK_C_QUEUE_NEED / RMK_C_PIECE_OVERFLOW, RMK_C_LIST_RESERVED, RMK_C_FLUSH_QUEUE_NEED: one copy, one wait
	if( !tail )
		HIPCHK( hipMemcpyAsync( sc->ctr(), sc->counters(), RMK_C_COPIED * sizeof( unsigned long long ), hipMemcpyDeviceToHost, sc->stream.get() ) );
	return 0;
}

static int launch_efn( rma_scanner_t *sc, int64_t count, const unsigned long long *n_dev, char *err, size_t errlen );

// The widths of the ordering's key fields for a database (DevHitSort::run).
struct KeyWidths { int seq, pos, rank; };
static KeyWidths key_widths( const rma_scanner_t *sc, const rma_db *db )
{
	return KeyWidths{ rma::bits_of( unsigned( db->n_seq > 0 ? db->n_seq - 1 : 0 ) ), rma::bits_of( unsigned( db->max_slen ) ),
		rma::bits_of( unsigned( sc->dprog.w_winsize ) ) };
}

// What plan_tail() needs of the scanner to say yes: the ordering's buffers for the hit buffer as it is, its work area and
// the staging buffer for n_sort records -- all of it before anything of the scan is enqueued.  false: no tail ahead.
static bool tail_room( rma_scanner_t *sc, const rma_db *db, int64_t n_sort, char *err, size_t errlen )
{
	const KeyWidths	w = key_widths( sc, db );
	if( sc->dsort.reserve( sc->hit_cap(), sc->dprog.hit_stride ) != hipSuccess || !sc->dsort.widths_ok( w.seq, w.pos, w.rank ) ||
		sc->dsort.plan( n_sort, sc->stream.get() ) != hipSuccess ){
		( void )hipGetLastError();
		return false;
	}
	return grow_h_raw( sc, size_t( n_sort ) * sc->dprog.hit_stride, err, errlen ) == 0;
}

// The tail of the scan in flight behind its search and drain kernels, sized by f.tail.n_sort on the host and by RMK_C_COUNT
// on the device: energies, ordering, the records' way back, and last the copy of the counters with the ordering's flag behind
// them -- rma_scan_end() waits once and reads what it needs to take the records or to do the tail again (tail_verdict).
static int launch_tail( rma_scanner_t *sc, char *err, size_t errlen )
{
	const rma_scanner::InFlight	&f = sc->fly;
	const int64_t	n_sort = f.tail.n_sort;
	const unsigned long long	*d_count = sc->counters() + RMK_C_COUNT;
	if( launch_efn( sc, n_sort, d_count, err, errlen ) )
		return 1;
	const KeyWidths	w = key_widths( sc, f.db );
	// (the gather kernel stores the records into the staging buffer as well: the copy back without a copy of its own)
	HIPCHK( sc->dsort.run( sc->hits(), n_sort, d_count, sc->counters() + rma_scanner::TAIL_FLAG, sc->raw(), w.seq, w.pos, w.rank, sc->stream.get() ) );
	HIPCHK( hipMemcpyAsync( sc->ctr(), sc->counters(), ( RMK_C_COPIED + 1 ) * sizeof( unsigned long long ), hipMemcpyDeviceToHost, sc->stream.get() ) );
	return 0;
}

// The [dbg] lines of the launch that has just ended (rm_scan_report.cpp), from a copy of the whole counter block.
static void debug_report( rma_scanner_t *sc )
{
	const rma_scanner::InFlight	&f = sc->fly;
	unsigned long long	ctr[ RMK_N_COUNTERS ] = { 0 };
	( void )hipMemcpy( ctr, sc->counters(), sizeof( ctr ), hipMemcpyDeviceToHost );
	rma::debug_report( ctr, rma::ScanShape{ sc->opt.dbg, f.lay->tile_t, f.plan.grouped ? f.lay->group : 1, f.lay->qcap, f.plan.grid, f.plan.lds,
		( long long )f.lay->n_tiles, f.plan.lean, sc->drained }, sc->dprog );
}

// The search kernel of a scan is on its way when this returns; rma_scan_end() (or search_finish())
// waits for it.  Two scanners that have begun run side by side on their own streams.
// (timed_apart: rma_scan_device() is the caller, which times the kernels apart: no tail behind the search kernel)
static int scan_begin( rma_scanner_t *sc, const rma_db_t *db, bool timed_apart, char *err, size_t errlen )
{
	HIPCHK( hipSetDevice( sc->device ) );
	if( sc->fly.db != nullptr ){
		snprintf( err, errlen, "rma_scan_begin: the scanner has a scan in flight (rma_scan_end() ends it)" );
		return 1;
	}
	if( db->device != sc->device ){
		snprintf( err, errlen, "the database lives on device %d, the scanner on device %d", db->device, sc->device );
		return 1;
	}
	if( sc->need_efn2 && !sc->d_efn2 ){
		snprintf( err, errlen, "the program has efn2() call sites but rma_scanner_set_efn2data() was not called" );
		return 1;
	}
	sc->d_last = nullptr;
	sc->n_last = 0;
	sc->last_state = 0;
	sc->last_relabelled = false;
	sc->end_waits = sc->search_launches = sc->efn_launches = 0;
	sc->tail_taken = false;
	const Layout	*lay = layout_for( sc, db, err, errlen );
	if( lay == nullptr )
		return 1;
	rma_scanner::InFlight	&f = sc->fly;
	f.db = db;
	f.lay = lay;
	{
		rma_db	*mdb = const_cast<rma_db *>( db );
		std::lock_guard<std::mutex>	lk( mdb->mu );
		mdb->busy.push_back( sc );
	}
	struct Unfly { rma_scanner *sc; bool armed; ~Unfly(){ if( armed ){
			rma_db	*mdb = const_cast<rma_db *>( sc->fly.db );
			std::lock_guard<std::mutex>	lk( mdb->mu );
			mdb->busy.erase( std::find( mdb->busy.begin(), mdb->busy.end(), sc ) );
			sc->fly.db = nullptr;
			sc->flying.lower();
		} } }	unfly{ sc, true };
	f.plan = rma::LaunchPlan();
	f.tail = rma::TailPlan();
	if( lay->n_tiles == 0 ){
		unfly.armed = false;
		return 0;
	}
	// (option beside at -1: room for the other scanner's drain kernel when another scanner of this device has a scan in
	// flight -- two scanners taking the steps in turns, from the second step on; this scan is not counted yet.  The shape
	// holds for the scan: search_finish()'s repeat launches read f.plan)
	rma::Options	opt = sc->opt;
	opt.beside = opt.beside < 0 ? rma::flights( sc->device ) > 0 : opt.beside;
	if( rma::plan_launch( *lay, lay->n_tiles, sc->plan, opt, sc->grid_blocks / 8, &f.plan, err, errlen ) )
		return 1;
	if( f.plan.pooled ){
		// The list of the drain kernel: room for an item per 32 bases (trna.descr leaves one per 70 before the
		// stem-loop tests and one per 4500 after them); a workgroup that finds it full walks its own items.
		int	want = !sc->opt.drain ? 0 : sc->opt.glist > 0 ? sc->opt.glist :
			int( std::min<long long>( std::max<long long>( db->sum_slen / 32, 1 << 18 ), 1 << 24 ) );
		if( lay->flush )		// (what an earlier scan reserved beyond the list's end: search_finish)
			want = std::max( want, sc->glist_need );
		const int	cap = sc->opt.pool_min + lay->qcap + sc->spill_cap();
		if( cap > sc->pool_cap || want > sc->glist_cap || ( want == 0 && sc->glist_cap != 0 ) || ( sc->opt.glist > 0 && want != sc->glist_cap && !lay->flush ) ){
			HIPCHK( hipStreamSynchronize( sc->stream.get() ) );
			if( grow_pool( sc, want, std::max( cap, sc->pool_cap ), err, errlen ) )
				return 1;
		}
	}
	// the database's upload and the tiling's, on the device's upload stream, come first
	HIPCHK( hipStreamWaitEvent( sc->stream.get(), db->ready.get(), 0 ) );
	HIPCHK( hipStreamWaitEvent( sc->stream.get(), lay->ready.get(), 0 ) );
	// the scan's tail behind its kernels, where the rule allows it and there is room (rm_tail_plan.h)
	f.tail = rma::plan_tail( sc->count_max, sc->hit_cap(), rma::TailOpts{ sc->opt.spec_tail, sc->opt.dbg, sc->opt.timing, sc->opt.host_sort, timed_apart } );
	if( f.tail.speculate && !tail_room( sc, db, f.tail.n_sort, err, errlen ) )
		f.tail = rma::TailPlan();
	sc->flying.raise( sc->device );		// (nothing is left that can refuse the scan; a launch that fails lowers it again: unfly)
	if( launch_search( sc, err, errlen, f.tail.speculate ) )
		return 1;
	if( f.tail.speculate && launch_tail( sc, err, errlen ) )
		return 1;
	unfly.armed = false;
	return 0;
}

extern "C" int rma_scan_begin( rma_scanner_t *sc, const rma_db_t *db, char *err, size_t errlen )
{
	return scan_begin( sc, db, false, err, errlen );
}

// Wait for the search kernel of the scan in flight; repeat it while it asks for a larger spill area
// or hit buffer (count-then-emit).  On return the candidates are in d_hits, unordered, no energies.
// (waited: the caller has waited for the stream and the counters of the first launch are on the host)
static int search_finish( rma_scanner_t *sc, int64_t *n_hits, float *search_ms, char *err, size_t errlen, bool waited = false )
{
	rma_scanner::InFlight	&f = sc->fly;
	*n_hits = 0;
	if( f.plan.grid == 0 )
		return 0;
	const rmd_program_t	&dp = sc->dprog;
	unsigned long long	count = 0;
	for( int attempt = 0; ; attempt++ ){
		if( !( waited && attempt == 0 ) ){
			HIPCHK( hipStreamSynchronize( sc->stream.get() ) );
			sc->end_waits++;
		}
		count = sc->ctr()[ RMK_C_COUNT ];
		if( sc->opt.dbg )
			debug_report( sc );
		bool	again = false;
		if( !f.plan.lean ){
			// the general instance does not search queue overflow in place: a larger spill area, and again
			const unsigned long long	need = sc->ctr()[ RMK_C_QUEUE_NEED ];
			if( need > 0 ){
				if( attempt == 3 ){
					snprintf( err, errlen, "work queue overflow after regrow (%llu items in a tile)", need );
					return 1;
				}
				if( grow_spill( sc, need, err, errlen ) )
					return 1;
				again = true;
			}
		}
		if( f.plan.walks_nothing ){
			// the instance that walks nothing reports what it had no room for -- a tile's items beyond queue and spill area, the
			// list's items beyond its end -- and the scan is repeated with room for them
			const unsigned long long	q_need = sc->ctr()[ RMK_C_FLUSH_QUEUE_NEED ], l_need = sc->ctr()[ RMK_C_LIST_RESERVED ];
			if( ( q_need > 0 || l_need > ( unsigned long long )sc->glist_cap ) && attempt == 3 ){
				snprintf( err, errlen, "work queue or item list overflow after regrow (%llu items in a tile, %llu in the list)", q_need, l_need );
				return 1;
			}
			if( q_need > 0 ){
				if( grow_spill( sc, q_need, err, errlen ) )
					return 1;
				again = true;
			}
			if( l_need > ( unsigned long long )sc->glist_cap ){
				if( l_need > ( 1ull << 28 ) ){
					snprintf( err, errlen, "%llu items for the drain kernel's list: more than it can be made to hold", l_need );
					return 1;
				}
				sc->glist_need = int( l_need + l_need / 8 ) + 1024;
				if( grow_pool( sc, sc->glist_need, sc->pool_cap, err, errlen ) )
					return 1;
				again = true;
			}
		}
		if( f.plan.lean && sc->ctr()[ RMK_C_PIECE_OVERFLOW ] != 0 && !sc->whole_items ){
			// a piece of an item found more candidates than the order words of the pieces leave room for
			// (PIECE_ORDER_BITS): once more, and from now on, with whole items
			sc->whole_items = true;
			again = true;
		}
		if( !again && int64_t( count ) > sc->hit_cap() ){
			if( attempt == 3 ){
				snprintf( err, errlen, "hit buffer overflow after regrow (%llu candidates)", count );
				return 1;
			}
			// count-then-emit: the first pass told us how many records there are
			HIPCHK( sc->d_hits.exact( ( size_t( count ) + 1024 ) * dp.hit_stride * sizeof( int32_t ) ) );
			again = true;
		}
		if( !again )
			break;
		if( launch_search( sc, err, errlen ) )
			return 1;
	}
	if( search_ms )
		HIPCHK( hipEventElapsedTime( search_ms, sc->ev[ 0 ].get(), sc->ev[ 1 ].get() ) );
	*n_hits = int64_t( count );
	return 0;
}

// n_dev: null, or the count on the device -- then `count` is what the grid is planned for and the kernels take
// min( *n_dev, the hit buffer's room ) records
static int launch_efn( rma_scanner_t *sc, int64_t count, const unsigned long long *n_dev, char *err, size_t errlen )
{
	const rmd_program_t	&dp = sc->dprog;
	if( !( ( sc->have_efn || sc->d_efn2 ) && dp.n_efn > 0 && count > 0 ) )
		return 0;
	sc->efn_launches++;
	// one workgroup per CU at most (its LDS), each striding over the candidates
	const int64_t	blocks = std::min<int64_t>( ( count + EFN_BLOCK - 1 ) / EFN_BLOCK, sc->grid_blocks / 8 );
	rmk_efn_args	a{ sc->d_prog.as<rmd_program_t>(), view_of( sc->fly.db, sc->fly.lay ), sc->hits(), ( long long )( n_dev != nullptr ? sc->hit_cap() : count ),
		sc->have_efn ? sc->d_t16.as<int16_t>() : nullptr, sc->d_tlkey.as<int32_t>(), sc->d_loginc.as<int32_t>(), sc->efn2(), n_dev };
	sc->efn_ran = true;
	HIPCHK( hipEventRecord( sc->ev[ 2 ].get(), sc->stream.get() ) );
	if( sc->fly.plan.efn_light )
		HIPCHK( rmk_launch_efn_light( int( std::min<int64_t>( ( count + 63 ) / 64, sc->grid_blocks * 2 ) ), sc->stream.get(), a ) );
	else
	HIPCHK( sc->dprog.efn_big ? rmk_launch_efn_big( int( blocks ), sc->stream.get(), a ) : rmk_launch_efn( int( blocks ), sc->stream.get(), a ) );
	HIPCHK( hipEventRecord( sc->ev[ 3 ].get(), sc->stream.get() ) );
	return 0;
}

static void scan_done( rma_scanner_t *sc )
{
	sc->flying.lower();
	if( sc->fly.db == nullptr )
		return;
	rma_db	*mdb = const_cast<rma_db *>( sc->fly.db );
	{
		std::lock_guard<std::mutex>	lk( mdb->mu );
		auto	it = std::find( mdb->busy.begin(), mdb->busy.end(), sc );
		if( it != mdb->busy.end() )
			mdb->busy.erase( it );
	}
	sc->fly.db = nullptr;
	sc->fly.lay = nullptr;
}

extern "C" int rma_scan_device( rma_scanner_t *sc, const rma_db_t *db, int64_t *n_hits, float *search_ms,
	float *efn_ms, char *err, size_t errlen )
{
	*n_hits = 0;
	if( search_ms ) *search_ms = 0;
	if( efn_ms ) *efn_ms = 0;
	if( scan_begin( sc, db, true, err, errlen ) )	// (the kernels timed apart: no tail behind the search kernel, one energy launch behind the wait)
		return 1;
	struct Done { rma_scanner *sc; ~Done(){ scan_done( sc ); } }	done{ sc };
	int64_t	n = 0;
	if( search_finish( sc, &n, search_ms, err, errlen ) )
		return 1;
	*n_hits = n;
	sc->count_max = rma::tail_seen( sc->count_max, n );
	const bool	has_efn = ( sc->have_efn || sc->d_efn2 ) && sc->dprog.n_efn > 0 && n > 0;
	if( launch_efn( sc, n, nullptr, err, errlen ) )
		return 1;
	HIPCHK( hipStreamSynchronize( sc->stream.get() ) );
	if( efn_ms && has_efn )
		HIPCHK( hipEventElapsedTime( efn_ms, sc->ev[ 2 ].get(), sc->ev[ 3 ].get() ) );
	return 0;
}

// The kernels of the scanner's last search, by HIP events on its stream: ms[ 0 ] the search kernel, ms[ 1 ] the
// drain kernel that walked what it left in the list (0: there was none), ms[ 2 ] the efn kernel (0: none).
extern "C" int rma_scanner_last_kernel_ms( rma_scanner_t *sc, float ms[ 3 ], char *err, size_t errlen )
{
	HIPCHK( hipSetDevice( sc->device ) );
	ms[ 0 ] = ms[ 1 ] = ms[ 2 ] = 0;
	HIPCHK( hipStreamSynchronize( sc->stream.get() ) );
	if( !sc->searched )
		return 0;		// (nothing was launched yet)
	if( sc->drained ){
		HIPCHK( hipEventElapsedTime( &ms[ 0 ], sc->ev[ 0 ].get(), sc->ev[ 4 ].get() ) );
		HIPCHK( hipEventElapsedTime( &ms[ 1 ], sc->ev[ 4 ].get(), sc->ev[ 1 ].get() ) );
	}else
		HIPCHK( hipEventElapsedTime( &ms[ 0 ], sc->ev[ 0 ].get(), sc->ev[ 1 ].get() ) );
	if( sc->efn_ran )
		HIPCHK( hipEventElapsedTime( &ms[ 2 ], sc->ev[ 2 ].get(), sc->ev[ 3 ].get() ) );
	return 0;
}

// The shape of the scanner's last search launch: out[ 0 ] workgroups asked for, out[ 1 ] bytes of dynamic LDS a workgroup,
// out[ 2 ] workgroups of the drain kernel behind it (0: none), out[ 3 ] 1 when the shape leaves another scanner's drain
// kernel room (option beside).  All 0 before the first launch.
extern "C" int rma_scanner_last_launch( rma_scanner_t *sc, int out[ 4 ] )
{
	for( int i = 0; i < 4; i++ )
		out[ i ] = sc->last_launch[ i ];
	return 0;
}

// What the scanner's last rma_scan_end() (or rma_scan(), rma_scan_end_on_device()) did: out[ 0 ] the times it waited for the
// stream, out[ 1 ] 1 when it took the records of the tail that rma_scan_begin() had enqueued ahead (rm_tail_plan.h), out[ 2 ]
// launches of the search kernel, out[ 3 ] launches of an energy kernel -- of the whole scan, from its begin.
extern "C" int rma_scanner_last_end( rma_scanner_t *sc, int out[ 4 ] )
{
	out[ 0 ] = sc->end_waits;
	out[ 1 ] = sc->tail_taken ? 1 : 0;
	out[ 2 ] = sc->search_launches;
	out[ 3 ] = sc->efn_launches;
	return 0;
}

// Energies, reference order, copy back.  With on_device_only the ordered records stay in HBM
// (rma_scanner::d_last, for rma_gather_hits) and *hits is not set.
static int scan_end( rma_scanner_t *sc, const int32_t **hits, int64_t *n_hits, bool copy_back, char *err, size_t errlen )
{
	*n_hits = 0;
	if( hits )
		*hits = nullptr;
	if( sc->fly.db == nullptr ){
		snprintf( err, errlen, "rma_scan_end: no scan in flight" );
		return 1;
	}
	HIPCHK( hipSetDevice( sc->device ) );
	struct Done { rma_scanner *sc; ~Done(){ scan_done( sc ); } }	done{ sc };
	const bool	timing = sc->opt.timing != 0;
	auto	t0 = std::chrono::steady_clock::now();
	auto lap = [&]( const char *what ){
		if( timing ){
			auto	t1 = std::chrono::steady_clock::now();
			fprintf( stderr, "[timing] %-10s %8.3f ms\n", what, std::chrono::duration<double, std::milli>( t1 - t0 ).count() );
			t0 = t1;
		}
	};
	int64_t	n = 0;
	const bool	ahead = sc->fly.tail.speculate;
	if( ahead ){
		// the tail was enqueued at rma_scan_begin: one wait, and the counters say whether its records are the scan's
		HIPCHK( hipStreamSynchronize( sc->stream.get() ) );
		sc->end_waits++;
		const rma_scanner::InFlight	&f = sc->fly;
		const unsigned long long	*c = sc->ctr(), count = c[ RMK_C_COUNT ];
		rma::TailRepeat	r;
		r.queue_need = !f.plan.lean && c[ RMK_C_QUEUE_NEED ] > 0;
		r.flush_queue_need = f.plan.walks_nothing && c[ RMK_C_FLUSH_QUEUE_NEED ] > 0;
		r.list_need = f.plan.walks_nothing && c[ RMK_C_LIST_RESERVED ] > ( unsigned long long )sc->glist_cap;
		r.piece_overflow = f.plan.lean && c[ RMK_C_PIECE_OVERFLOW ] != 0 && !sc->whole_items;
		if( rma::tail_verdict( count, f.tail.n_sort, sc->hit_cap(), r, c[ rma_scanner::TAIL_FLAG ] != 0, int64_t( count ) ) == rma::TAIL_TAKE ){
			n = int64_t( count );
			*n_hits = n;
			sc->count_max = rma::tail_seen( sc->count_max, n );
			sc->tail_taken = true;
			sc->d_last = sc->dsort.d_out();
			sc->n_last = n;
			sc->last_state = 1;
			if( hits )
				*hits = copy_back ? sc->raw() : nullptr;
			return 0;
		}
		// not taken: on from here as without a tail ahead -- the energies again, which are written from a record's other words
	}
	if( search_finish( sc, &n, nullptr, err, errlen, ahead ) )
		return 1;
	lap( "search" );
	*n_hits = n;
	sc->count_max = rma::tail_seen( sc->count_max, n );
	sc->last_state = 1;		// (no records: nothing to be anywhere)
	if( n == 0 ){
		sc->efn_ran = false;	// (an energy kernel of a tail ahead had nothing to do)
		return 0;
	}
	sc->last_state = 2;		// (until the ordered records are known to be in HBM)
	if( launch_efn( sc, n, nullptr, err, errlen ) )
		return 1;
	if( timing ){
		HIPCHK( hipStreamSynchronize( sc->stream.get() ) );
		sc->end_waits++;
		lap( "energies" );
	}
	const rma_db	*db = sc->fly.db;
	const int	stride = sc->dprog.hit_stride;
	const size_t	words = size_t( n ) * stride;
	if( copy_back && grow_h_raw( sc, words, err, errlen ) )
		return 1;
	// Reference order -- (entry, strand, start, rank, order), order word renumbered -- on the device,
	// behind the efn kernel on the same stream: what comes back is the final stream (rm_hitsort_dev.h).
	// Header words that do not fit the 64-bit key (or host_sort): the host's sort_hits().
	bool	on_device = false;
	if( !sc->opt.host_sort && n >= 2 ){
		if( sc->dsort.reserve( sc->hit_cap(), stride ) == hipSuccess &&
			sc->dsort.run( sc->hits(), n, rma::bits_of( unsigned( db->n_seq > 0 ? db->n_seq - 1 : 0 ) ), rma::bits_of( unsigned( db->max_slen ) ),
				rma::bits_of( unsigned( sc->dprog.w_winsize ) ), sc->stream.get() ) == hipSuccess ){
			if( timing ){
				HIPCHK( hipStreamSynchronize( sc->stream.get() ) );
				sc->end_waits++;
				lap( "sorted" );
			}
			if( copy_back )
				HIPCHK( hipMemcpyAsync( sc->raw(), sc->dsort.d_out(), words * sizeof( int32_t ), hipMemcpyDeviceToHost, sc->stream.get() ) );
			HIPCHK( hipMemcpyAsync( sc->ctr(), sc->dsort.d_flag(), sizeof( unsigned long long ), hipMemcpyDeviceToHost, sc->stream.get() ) );
			HIPCHK( hipStreamSynchronize( sc->stream.get() ) );
			sc->end_waits++;
			on_device = sc->ctr()[ 0 ] != sc->dsort.epoch;	// (raised: the word holds this run's number, rm_hitsort_dev.h)
			if( !on_device && sc->dsort.w_ord < 31 )
				sc->dsort.w_ord = 31;	// (order words above 255: room for them from now on, if the other fields leave it)
		}else
			( void )hipGetLastError();
	}
	if( on_device ){
		lap( "ordered" );
		sc->d_last = sc->dsort.d_out();
		sc->n_last = n;
		sc->last_state = 1;
		if( hits )
			*hits = copy_back ? sc->raw() : nullptr;
		return 0;
	}
	if( n == 1 && !sc->opt.host_sort ){
		// (a single record is in order; its order word -- the kernels leave the number of the walk's choices
		// there, or a count within a piece of an item -- is 0 as the sorts would make it)
		HIPCHK( hipMemsetAsync( sc->hits() + 4, 0, sizeof( int32_t ), sc->stream.get() ) );
		if( copy_back )
			HIPCHK( hipMemcpyAsync( sc->raw(), sc->hits(), words * sizeof( int32_t ), hipMemcpyDeviceToHost, sc->stream.get() ) );
		HIPCHK( hipStreamSynchronize( sc->stream.get() ) );
		sc->end_waits++;
		sc->d_last = sc->hits();
		sc->n_last = 1;
		sc->last_state = 1;
		if( hits )
			*hits = copy_back ? sc->raw() : nullptr;
		return 0;
	}
	if( grow_h_raw( sc, words, err, errlen ) )		// (not asked to copy back, but the host has to order)
		return 1;
	HIPCHK( hipMemcpyAsync( sc->raw(), sc->hits(), words * sizeof( int32_t ), hipMemcpyDeviceToHost, sc->stream.get() ) );
	HIPCHK( hipStreamSynchronize( sc->stream.get() ) );
	sc->end_waits++;
	lap( "copy back" );
	sc->h_sorted.resize( words );
	rma::sort_hits( sc->raw(), n, stride, sc->h_sorted.data(), sc->keys, sc->keys_tmp );
	lap( "ordering" );
	if( !copy_back ){
		// the ordered records back where a device-side consumer finds them
		HIPCHK( hipMemcpyAsync( sc->hits(), sc->h_sorted.data(), words * sizeof( int32_t ), hipMemcpyHostToDevice, sc->stream.get() ) );
		HIPCHK( hipStreamSynchronize( sc->stream.get() ) );
		sc->end_waits++;
		sc->d_last = sc->hits();
		sc->n_last = n;
		sc->last_state = 1;
	}
	// (copy_back with the ordering on the host: the ordered records are on the host only, last_state stays 2 and
	// rma_gather_hits() says so instead of sending nothing)
	if( hits )
		*hits = sc->h_sorted.data();
	return 0;
}

extern "C" int rma_scan_end( rma_scanner_t *sc, const int32_t **hits, int64_t *n_hits, char *err, size_t errlen )
{
	return scan_end( sc, hits, n_hits, true, err, errlen );
}

extern "C" int rma_scan( rma_scanner_t *sc, const rma_db_t *db, const int32_t **hits, int64_t *n_hits,
	char *err, size_t errlen )
{
	*hits = nullptr;
	*n_hits = 0;
	if( rma_scan_begin( sc, db, err, errlen ) )
		return 1;
	return scan_end( sc, hits, n_hits, true, err, errlen );
}

// the ordered records of a scan left in HBM (for a collective that sends them from there)
extern "C" int rma_scan_end_on_device( rma_scanner_t *sc, const int32_t **d_hits, int64_t *n_hits, char *err, size_t errlen )
{
	*d_hits = nullptr;
	if( scan_end( sc, nullptr, n_hits, false, err, errlen ) )
		return 1;
	*d_hits = *n_hits > 0 ? sc->d_last : nullptr;
	return 0;
}

// The last scan's ordered records into caller device memory: the copy on the scanner's stream, between the
// caller's stream and the scanner's both ways (behind what the caller has queued that may still use dst,
// ahead of the caller's next work and of the scanner's next scan).
extern "C" int rma_scan_records_to_device( rma_scanner_t *sc, int32_t *dst, int64_t dst_words, void *stream, char *err, size_t errlen )
{
	if( sc->last_state != 1 ){
		snprintf( err, errlen, "rma_scan_records_to_device: %s", sc->last_state == 0 ? "no scan has ended" :
			"the last scan's records are on the host only (end the scan with rma_scan_end_on_device)" );
		return 1;
	}
	const int64_t	words = sc->n_last * sc->dprog.hit_stride;
	if( dst_words < words ){
		snprintf( err, errlen, "rma_scan_records_to_device: %lld words of records, room for %lld", ( long long )words, ( long long )dst_words );
		return 1;
	}
	if( words == 0 )
		return 0;
	HIPCHK( hipSetDevice( sc->device ) );
	if( rma::check_device_bytes( dst, sc->device, 0, words * 4, "the destination", err, errlen ) )
		return 1;
	hipStream_t	caller = static_cast<hipStream_t>( stream );
	if( rma::stream_after( sc->stream.get(), caller, err, errlen ) )
		return 1;
	HIPCHK( hipMemcpyAsync( dst, sc->d_last, size_t( words ) * 4, hipMemcpyDeviceToDevice, sc->stream.get() ) );
	return rma::stream_after( caller, sc->stream.get(), err, errlen );
}

// One scan of eight start positions, so that what the runtime sets up on first use (code objects of
// the kernel instance this descriptor takes, the first device allocations of a database, the ordering's
// kernels) is paid before the first batch of a search: 15-50 ms there.  All 'a': for most
// descriptors nothing pairs; whatever is found is thrown away.  Called by the command line program
// once the scanner is complete (efn2 tables attached); the library never runs it by itself.
extern "C" int rma_scanner_warmup( rma_scanner_t *sc, char *err, size_t errlen )
{
	if( sc->prog.dminlen > 2000 )
		return 0;
	HIPCHK( hipSetDevice( sc->device ) );
	const rma::Options	keep = sc->opt;
	sc->opt.dbg = 0;		// (no diagnostics of the warm-up)
	sc->opt.timing = 0;
	const std::string	warm( size_t( std::max( sc->prog.dminlen, 1 ) + 7 ), 'a' );
	const char	*seqs[ 1 ] = { warm.c_str() };
	const int32_t	lens[ 1 ] = { int32_t( warm.size() ) };
	rma_db_t	*wdb = nullptr;
	int	rc = rma_db_create( sc, seqs, lens, 1, &wdb, err, errlen );
	if( rc == 0 ){
		const int32_t	*wh = nullptr;
		int64_t	wn = 0;
		rc = rma_scan( sc, wdb, &wh, &wn, err, errlen );
		rma_db_destroy( wdb );
	}
	if( sc->dprog.n_efn > 0 ){
		// ... and the energy kernel, which the scan above did not reach (no candidate): one launch over no
		// records -- its code object, and the scratch memory its interval stack makes the runtime set
		// aside at a kernel's first launch (9 ms in the first batch, measured)
		( void )rmk_preload_efn();
		rmk_efn_args	a{ sc->d_prog.as<rmd_program_t>(), DbView{}, sc->hits(), 0ll, sc->have_efn ? sc->d_t16.as<int16_t>() : nullptr, sc->d_tlkey.as<int32_t>(),
			sc->d_loginc.as<int32_t>(), sc->efn2() };
		( void )rmk_launch_efn( 1, sc->stream.get(), a );
		( void )hipStreamSynchronize( sc->stream.get() );
		( void )hipGetLastError();
	}
	if( rc == 0 && sc->dsort.cap >= 16384 ){
		// ... and a pass of the ordering over a cleared hit buffer at either size: its own sort of a few thousand records, the library's
		( void )hipMemsetAsync( sc->hits(), 0, size_t( 16384 ) * sc->dprog.hit_stride * sizeof( int32_t ), sc->stream.get() );
		( void )sc->dsort.run( sc->hits(), 16384, 10, 20, 8, sc->stream.get() );
		( void )sc->dsort.run( sc->hits(), 4096, 10, 20, 8, sc->stream.get() );
		// ... and the way back of the records, as a scan ends: the first copy of this size from the device
		// sets up the engine that makes it
		if( sc->h_raw_cap() >= size_t( 4096 ) * sc->dprog.hit_stride )
			( void )hipMemcpyAsync( sc->raw(), sc->dsort.d_out(), size_t( 4096 ) * sc->dprog.hit_stride * sizeof( int32_t ), hipMemcpyDeviceToHost, sc->stream.get() );
		( void )hipStreamSynchronize( sc->stream.get() );
		( void )hipGetLastError();
	}
	sc->opt = keep;
	sc->count_max = -1;		// (the warm-up is not a scan the tail is planned from)
	return rc;
}
