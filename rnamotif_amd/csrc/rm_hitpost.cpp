// rm_hitpost.cpp -- the calls of the C ABI (include/rnamotif_amd.h) that consume hit records already on the device,
// on the host: rma_hit_windows (the device half of rma_replay_device), rma_hit_structures, rma_hit_alignment and
// rma_prune_hits.  Their kernels are rm_hitwin_dev.hip, rm_hitstruct_dev.hip, rm_hitalign_dev.hip and rm_prune_dev.hip.
// Behind them rma_structure_energies (rm_structenergy_dev.hip), which consumes what rma_hit_structures makes -- or any
// structures in device memory -- and rma_scanner_load_energy_tables, which gives a scanner the tables for it.
// Of a scan they need nothing: a scanner's program and device, a database's tables and text (rm_scanner_impl.h), and
// scratch of their own.  Last rma_score_hits (rm_score_dev.hip): the score section's MAIN over records, the rule of
// rm_score_core.h on an image of rm_score_image.h -- and, for the records of a loose descriptor ahead of it,
// rma_seqcheck_hits (rm_seqcheck_dev.hip): the seq= expressions themselves, the rule of rm_seqcheck.h.  At the end of
// the chain rma_hit_print (rm_hitprint_dev.hip): the records and their score columns as the lines rnamotif prints, the
// rule of rm_hitprint.h, with the entries' names from a table rma_names_create puts on the device -- and beside it
// rma_hit_list (rm_hitlist_dev.hip): the same records as rmfmt lists them, sorted and in columns, the rule of
// rm_hitlist.h -- and rma_hit_ct (rm_hitct_dev.hip): the same records as rm2ct writes them, the rule of rm_hitct.h.
// The file also holds what the calls are given besides records: rma_names_* (the entries' names on the device) and
// rma_scanner_load_energy_tables.  What the calls all do first is written once:
//   record_call_args    the database, the records and the device refused or accepted
//   letters_on_device   the table the window bytes go through
//   check_records       behind the caller's stream, the bad-record word reset, every record judged by the span kernel
// The refusal words of the span scratch, which several calls share, are named in rm_hitpost.h (HitBadSlot on the
// device, HitBadHostSlot page-locked), and the scratch is carved for as many as are named.
#include <algorithm>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>
#include "rm_scanner_impl.h"
#include "rm_hitpost.h"
#include "rm_hitwin_dev.h"
#include "rm_hitstruct_dev.h"
#include "rm_hitalign_dev.h"
#define RMD_FN		static inline
#define RMD_FN_MEMBER	inline
#include "rm_hitprint_dev.h"
#include "rm_hitlist_dev.h"
#include "rm_hitct_dev.h"
#include "rm_structenergy.h"
#include "rm_structenergy_dev.h"
#include "rm_score_core.h"
#include "rm_score_dev.h"
#include "rm_seqcheck.h"
#include "rm_seqcheck_dev.h"

namespace {
// records of a call go through the kernels HW_CHUNK at a time; windows come to the host (rma_hit_windows) in pieces
// of at most HW_PIECE_WINDOW bytes of windows and HW_PIECE_RECORDS bytes of records (a longer window comes alone)
constexpr int64_t	HW_CHUNK = int64_t( 1 ) << 17;
constexpr int64_t	HW_PIECE_WINDOW = int64_t( 16 ) << 20, HW_PIECE_RECORDS = int64_t( 8 ) << 20;

}	// namespace

// the two fixed blocks (rm_hitpost.h), the scan's room, windows; page-locked: the fixed block, records, windows
struct rma::HitWindowScratch : rma::HitWinFixed {
	int	device = -1;
	Stream	stream;
	DevMem	d_fixed, d_tmp, d_win;
	PinMem	h_fixed, h_rec, h_win;
	std::vector<int64_t>	piece_off;
};

void rma::hitwin_scratch_free( HitWindowScratch *s )
{
	if( s == nullptr )
		return;
	( void )hipSetDevice( s->device );
	if( s->stream.get() != nullptr )
		( void )hipStreamSynchronize( s->stream.get() );
	delete s;
}

// What a scanner keeps for these calls, made by the first that needs it.  Each call's fixed pieces are there together or
// not at all (its first use builds them in locals and moves them in); the pieces that grow are asked for room per call.
struct rma::HitPost {
	// rma_hit_structures, rma_hit_alignment: the span scratch and stream, the program's table and, behind it, the running total
	HitWindowScratch	*win = nullptr;
	DevMem	hs;
	static constexpr size_t	HS_CARRY_AT = ( sizeof( HitStructTable ) + 7 ) & ~size_t( 7 );
	HitStructTable	*hs_table() const { return hs.as<HitStructTable>(); }
	int64_t	*hs_carry() const { return reinterpret_cast<int64_t *>( hs.as<char>() + HS_CARRY_AT ); }
	// rma_prune_hits: the program's table (two result words behind it), two page-locked words and the event behind the
	// last call's kernels; the keys, flags and block list of a call, the entries' name groups
	DevMem	pr_table;
	PinMem	h_pr;
	Event	pr_done;
	DevMem	d_pr, d_pr_groups;
	// rma_structure_energies: two result words and the 256 codes of a call's bytes (device and page-locked) and the
	// event behind the last call's kernels; the info word of every structure of a call
	DevMem	d_se;
	PinMem	h_se;
	Event	se_done;
	DevMem	d_se_info;
	// rma_score_hits: two result words, a stopped record's result and a call's accept flags, kinds and scores; two
	// page-locked words and a result; the image that is on the device now (its serial; 0: none) and its bytes
	// (behind the image's bytes the table of bits() of an image with text; d_sc_heap: the records' heaps of one chunk)
	DevMem	d_sc, d_sc_image, d_sc_heap;
	PinMem	h_sc;
	uint64_t	sc_serial = 0;
	// rma_seqcheck_hits: two result words, a stopped record's result and a call's keep flags and fixed rows; two
	// page-locked words and a result; the image that is on the device now (its serial; 0: none) and its bytes
	DevMem	d_sq, d_sq_image;
	PinMem	h_sq;
	uint64_t	sq_serial = 0;
	// rma_hit_list: the fixed block (a call's sums, layout and letters) on the device and page-locked; the measured
	// records, the printed records' indices and the sort's work area of a call
	DevMem	d_hl, d_hl_rec, d_hl_idx, d_hl_tmp;
	PinMem	h_hl;
};

// (the scanner's device is current; the scratch stream is synchronised before anything goes)
void rma::hitpost_free( HitPost *p )
{
	if( p == nullptr )
		return;
	hitwin_scratch_free( p->win );
	delete p;
}

static rma::HitPost &post_of( rma_scanner_t *sc )
{
	if( sc->post == nullptr )
		sc->post = new rma::HitPost;
	return *sc->post;
}

// *scratch is a complete scratch on `device`: the one that is there, or a new one in its place
static int scratch_on( rma::HitWindowScratch **scratch, int device, char *err, size_t errlen )
{
	if( *scratch != nullptr && ( *scratch )->device == device )
		return 0;
	rma::hitwin_scratch_free( *scratch );
	*scratch = nullptr;
	std::unique_ptr<rma::HitWindowScratch, void ( * )( rma::HitWindowScratch * )>	made( new rma::HitWindowScratch, rma::hitwin_scratch_free );
	rma::HitWindowScratch	*s = made.get();
	s->device = device;
	HIPCHK( s->stream.create( hipStreamNonBlocking ) );
	HIPCHK( s->d_fixed.room( s->carve_dev( nullptr, size_t( HW_CHUNK ) ) ) );
	s->carve_dev( s->d_fixed.as<void>(), size_t( HW_CHUNK ) );
	size_t	tmp = 0;
	HIPCHK( rma::hit_offsets( s->d_len, s->d_off, HW_CHUNK + 1, nullptr, &tmp, s->stream.get() ) );
	HIPCHK( s->d_tmp.room( std::max<size_t>( tmp, 256 ) ) );
	HIPCHK( s->h_fixed.room( s->carve_host( nullptr, size_t( HW_CHUNK ) ) ) );
	s->carve_host( s->h_fixed.as<void>(), size_t( HW_CHUNK ) );
	*scratch = made.release();
	return 0;
}

// ---------------------------------------------------------------- what every call does first
namespace {

struct RecordCall {
	const char	*who;		// the prefix of every refusal
	int	device;			// the scanner's, which must be the database's; < 0: a call without a scanner, which takes the
					// database's and touches no device for no records (rma_replay_device)
	bool	device_db;		// the database must be one rma_db_create_device() made, not yet destroyed, whose text is read
	int64_t	most;			// records: more would overflow a byte count of the call
};

// The single argument check.  Passed with n_hits > 0: the database's device is current, the n_hits records of
// `stride` words lie inside their allocation on it.
int record_call_args( const RecordCall &c, const rma_db *db, int stride, const int32_t *d_hits, int64_t n_hits, char *err, size_t errlen )
{
	if( c.device_db && !rma::is_device_db( db ) ){
		snprintf( err, errlen, "%s: the database (%p) was not made by rma_db_create_device() or has been destroyed", c.who,
			static_cast<const void *>( db ) );
		return 1;
	}
	if( n_hits < 0 || ( n_hits > 0 && d_hits == nullptr ) || n_hits > c.most ){
		snprintf( err, errlen, "%s: %lld records: bad arguments", c.who, ( long long )n_hits );
		return 1;
	}
	if( c.device >= 0 && db->device != c.device ){
		snprintf( err, errlen, "%s: the database is on device %d, the scanner on device %d", c.who, db->device, c.device );
		return 1;
	}
	if( n_hits == 0 && c.device < 0 )
		return 0;
	HIPCHK( hipSetDevice( db->device ) );
	if( n_hits == 0 )
		return 0;
	if( rma::check_device_bytes( d_hits, db->device, 0, n_hits * stride * 4, "the records", err, errlen ) )
		return 1;
	if( c.device_db && db->text_hi > db->text_lo &&
		rma::check_device_bytes( db->text, db->device, db->text_lo, db->text_hi, "the database's text", err, errlen ) )
		return 1;
	return 0;
}

// The letters of window bytes: the caller's 256, the readers', or the letters of the database's own codes (*codes = 1,
// its table on the device); the first two on their way to the scratch's table on its stream.
int letters_on_device( rma::HitWindowScratch *s, const rma_db *db, const uint8_t *letters, const uint8_t **tab, int *codes, char *err, size_t errlen )
{
	*tab = s->d_tab;
	*codes = 0;
	if( letters != nullptr )
		memcpy( s->h_tab, letters, 256 );
	else if( db->default_table )
		for( int b = 0; b < 256; b++ )
			s->h_tab[ b ] = rma::hitwin_reader_letter( static_cast<unsigned char>( b ) );
	else{
		*tab = db->d_table;
		*codes = 1;
		return 0;
	}
	HIPCHK( hipMemcpyAsync( s->d_tab, s->h_tab, 256, hipMemcpyHostToDevice, s->stream.get() ) );
	return 0;
}

// The record check, queued on the scratch's stream behind the caller's work on its stream (the records) and the
// database's tables: d_bad[ HB_RECORD ] -- the least index of a bad record -- reset, zero_bytes bytes at `zero` (the
// call's running result; may be null) cleared, and, with `whole`, every record judged by the span kernel, which writes
// nothing else.  The caller queues its own kernels, copies the word back with its result and synchronises once.
int check_records( rma::HitWindowScratch *s, const rma_db *db, const rma_program_t &prog, const int32_t *d_hits, int64_t n_hits,
	void *stream, bool whole, void *zero, size_t zero_bytes, char *err, size_t errlen )
{
	hipStream_t	st = s->stream.get();
	if( rma::stream_after( st, static_cast<hipStream_t>( stream ), err, errlen ) )
		return 1;
	HIPCHK( hipStreamWaitEvent( st, db->ready.get(), 0 ) );
	HIPCHK( hipMemsetAsync( s->d_bad + rma::HB_RECORD, 0xff, sizeof( unsigned long long ), st ) );
	if( zero != nullptr )
		HIPCHK( hipMemsetAsync( zero, 0, zero_bytes, st ) );
	if( whole )
		HIPCHK( rma::hit_spans( d_hits, n_hits, rma_hit_stride( &prog ), rma::hitwin_shape( prog ), db->d_slen, db->d_text_start, db->n_seq,
			nullptr, nullptr, nullptr, s->d_bad + rma::HB_RECORD, st ) );
	return 0;
}

}	// namespace

// the words of a bad record, why it is bad; tab: the helix check as well (rma_hit_structures); nothing: "printed" or "written"
static int bad_record( rma::HitWindowScratch *s, const rma_db *db, const rma_program_t &prog, const int32_t *d_hits, int64_t h,
	const rma::HitStructTable *tab, const char *nothing, char *err, size_t errlen )
{
	const int	stride = rma_hit_stride( &prog );
	std::vector<int32_t>	w( static_cast<size_t>( stride ) );
	HIPCHK( hipMemcpyAsync( w.data(), d_hits + h * stride, size_t( stride ) * 4, hipMemcpyDeviceToHost, s->stream.get() ) );
	HIPCHK( hipStreamSynchronize( s->stream.get() ) );
	int32_t	lo, hi;
	int	which;
	const rma::HitWinShape	shape = rma::hitwin_shape( prog );
	const int	r = tab != nullptr ? rma::hitstruct_check( w.data(), *tab, shape, db->n_seq, db->h_slen.data(), &lo, &hi, &which ) :
		rma::hitwin_span( w.data(), shape, db->n_seq, db->h_slen.data(), &lo, &hi, &which );
	if( r == rma::HW_ENTRY )
		snprintf( err, errlen, "record %lld: entry %d outside [0, %d): nothing %s", ( long long )h, w[ 0 ], db->n_seq, nothing );
	else if( r == rma::HW_STRAND )
		snprintf( err, errlen, "record %lld: strand %d, not 0 or 1: nothing %s", ( long long )h, w[ 1 ], nothing );
	else if( r == rma::HS_HELIX ){
		const int	first = tab->e[ which ].strand[ 0 ];
		snprintf( err, errlen, "record %lld: element %d has length %d, element %d of the same helix length %d: nothing %s", ( long long )h,
			which, w[ RMA_HIT_HDR + 4 * which + 1 ], first, w[ RMA_HIT_HDR + 4 * first + 1 ], nothing );
	}
	else if( r == rma::HW_EXTENT ){
		const int	k = which < shape.n_elems ? RMA_HIT_HDR + 4 * which : which == shape.n_elems ? shape.ctx_off : shape.ctx_off + 2;
		char	what[ 32 ];
		if( which < shape.n_elems )
			snprintf( what, sizeof( what ), "element %d", which );
		else
			snprintf( what, sizeof( what ), "the %s context", which == shape.n_elems ? "left" : "right" );
		snprintf( err, errlen, "record %lld: %s at offset %d, length %d, outside entry %d's %d bases: nothing %s", ( long long )h,
			what, w[ k ], w[ k + 1 ], w[ 0 ], db->h_slen[ size_t( w[ 0 ] ) ], nothing );
	}else
		snprintf( err, errlen, "record %lld: refused on the device, not on the host (records changed during the call?)", ( long long )h );
	return 1;
}

// ---------------------------------------------------------------- windows of hits of device databases
// The device half of rma_replay_device() (rm_capi.cpp has the replay): the records are checked and their windows
// cut out of the database's text on the device (rm_hitwin_dev.hip), in chunks of HW_CHUNK records, and come to
// the host in pieces.  One synchronisation learns a chunk's offsets (and, in the first chunk, whether some
// record is bad), one per piece ends its copy.
int rma_hit_windows( rma::HitWindowScratch **scratch, const rma_db *db, const rma_program_t &prog, const int32_t *d_hits,
	int64_t n_hits, const uint8_t *letters, void *stream, const std::function<void( const rma::HitWindowPiece & )> &each,
	char *err, size_t errlen )
{
	const int	stride = rma_hit_stride( &prog );
	// (n_hits * stride * 4: the bytes of the records)
	const RecordCall	call{ "rma_replay_device", -1, true, INT64_MAX / 4 / stride };
	if( record_call_args( call, db, stride, d_hits, n_hits, err, errlen ) )
		return 1;
	if( n_hits == 0 )
		return 0;
	if( scratch_on( scratch, db->device, err, errlen ) )
		return 1;
	rma::HitWindowScratch	*s = *scratch;
	hipStream_t	st = s->stream.get();
	const rma::HitWinShape	shape = rma::hitwin_shape( prog );
	const uint8_t	*tab = nullptr;
	int	codes = 0;
	if( letters_on_device( s, db, letters, &tab, &codes, err, errlen ) )
		return 1;
	// every record checked before any text is read: all of them here when there is more than one chunk, else
	// the first chunk's spans do it
	if( check_records( s, db, prog, d_hits, n_hits, stream, n_hits > HW_CHUNK, nullptr, 0, err, errlen ) )
		return 1;
	const int64_t	piece_records = std::max<int64_t>( 1, HW_PIECE_RECORDS / ( 4 * stride ) );
	for( int64_t c0 = 0; c0 < n_hits; c0 += HW_CHUNK ){
		const int64_t	cn = std::min( HW_CHUNK, n_hits - c0 );
		const int32_t	*ch = d_hits + c0 * stride;
		HIPCHK( rma::hit_spans( ch, cn, stride, shape, db->d_slen, db->d_text_start, db->n_seq, s->d_lo, s->d_len, s->d_src,
			s->d_bad + rma::HB_RECORD, st ) );
		size_t	tb = s->d_tmp.bytes();
		HIPCHK( rma::hit_offsets( s->d_len, s->d_off, cn + 1, s->d_tmp.as<void>(), &tb, st ) );
		HIPCHK( hipMemcpyAsync( s->h_off, s->d_off, size_t( cn + 1 ) * 8, hipMemcpyDeviceToHost, st ) );
		HIPCHK( hipMemcpyAsync( s->h_lo, s->d_lo, size_t( cn ) * 4, hipMemcpyDeviceToHost, st ) );
		if( c0 == 0 )
			HIPCHK( hipMemcpyAsync( s->h_bad + rma::HBH_FIRST, s->d_bad + rma::HB_RECORD, sizeof( unsigned long long ), hipMemcpyDeviceToHost, st ) );
		HIPCHK( hipStreamSynchronize( st ) );
		if( c0 == 0 && s->h_bad[ rma::HBH_FIRST ] != ~0ull )
			return bad_record( s, db, prog, d_hits, int64_t( s->h_bad[ rma::HBH_FIRST ] ), nullptr, "printed", err, errlen );
		for( int64_t a = 0; a < cn; ){
			int64_t	b = a + 1;
			while( b < cn && b - a < piece_records && s->h_off[ b + 1 ] - s->h_off[ a ] <= HW_PIECE_WINDOW )
				b++;
			const int64_t	bytes = s->h_off[ b ] - s->h_off[ a ];
			HIPCHK( s->d_win.room( size_t( std::max<int64_t>( bytes, 256 ) ) ) );
			HIPCHK( s->h_win.room( size_t( std::max<int64_t>( bytes, 256 ) ) ) );
			HIPCHK( s->h_rec.room( size_t( b - a ) * stride * 4 ) );
			HIPCHK( rma::hit_gather( db->text, b - a, s->d_src + a, s->d_off + a, tab, codes, s->d_win.as<uint8_t>(), st ) );
			HIPCHK( hipMemcpyAsync( s->h_rec.as<void>(), ch + a * stride, size_t( b - a ) * stride * 4, hipMemcpyDeviceToHost, st ) );
			if( bytes > 0 )
				HIPCHK( hipMemcpyAsync( s->h_win.as<void>(), s->d_win.as<void>(), size_t( bytes ), hipMemcpyDeviceToHost, st ) );
			HIPCHK( hipStreamSynchronize( st ) );
			s->piece_off.resize( size_t( b - a + 1 ) );
			for( int64_t i = a; i <= b; i++ )
				s->piece_off[ size_t( i - a ) ] = s->h_off[ i ] - s->h_off[ a ];
			each( rma::HitWindowPiece{ s->h_rec.as<int32_t>(), c0 + a, b - a, s->h_win.as<char>(),
				s->piece_off.data(), s->h_lo + a, db->h_slen.data(), db->n_seq } );
			a = b;
		}
	}
	return 0;
}

// ---------------------------------------------------------------- hit structures as device tensors
// rma_hit_structures_size() / rma_hit_structures(): the spans, sources and offsets of rm_hitwin_dev.hip in chunks of
// HW_CHUNK records, the helix check and the fill kernel of rm_hitstruct_dev.hip.  The outputs are the caller's and are
// written in place: a chunk's offsets count from its first record (the scan's), the window bytes of the chunks
// before it wait in a word on the device (*d_hs_carry), so no chunk needs the host.  The work runs on a stream of the
// scanner's own, behind the caller's stream and, when something was written, ahead of what the caller queues next.
namespace {

// What the calls for structures and alignments do first: the database, the records and the scanner's scratch (made on
// first use).  n_hits == 0 needs none of it.
int hit_structures_args( rma_scanner_t *sc, const rma_db *db, const int32_t *d_hits, int64_t n_hits, const char *who, char *err, size_t errlen )
{
	const int	stride = rma_hit_stride( &sc->prog );
	// (n_hits * stride * 4 bytes of records, ( n_hits + 1 ) * 8 of offsets)
	const RecordCall	call{ who, sc->device, true, INT64_MAX / 16 / stride };
	if( record_call_args( call, db, stride, d_hits, n_hits, err, errlen ) )
		return 1;
	if( n_hits == 0 )
		return 0;
	rma::HitPost	&p = post_of( sc );
	if( scratch_on( &p.win, sc->device, err, errlen ) )
		return 1;
	if( !p.hs ){
		// the program's table and, behind it, the running total
		const rma::HitStructTable	tab = rma::hitstruct_table( sc->prog );
		rma::DevMem	m;
		HIPCHK( m.exact( rma::HitPost::HS_CARRY_AT + sizeof( int64_t ) ) );
		HIPCHK( hipMemcpy( m.as<void>(), &tab, sizeof( tab ), hipMemcpyHostToDevice ) );
		p.hs = std::move( m );
	}
	return 0;
}

// One chunk's spans, sources and offsets into the scratch; *bad as hit_spans
int hit_structures_spans( rma_scanner_t *sc, const rma_db *db, const int32_t *ch, int64_t cn, unsigned long long *bad, char *err, size_t errlen )
{
	rma::HitWindowScratch	*s = sc->post->win;
	HIPCHK( rma::hit_spans( ch, cn, rma_hit_stride( &sc->prog ), rma::hitwin_shape( sc->prog ), db->d_slen, db->d_text_start, db->n_seq,
		s->d_lo, s->d_len, s->d_src, bad, s->stream.get() ) );
	size_t	tb = s->d_tmp.bytes();
	HIPCHK( rma::hit_offsets( s->d_len, s->d_off, cn + 1, s->d_tmp.as<void>(), &tb, s->stream.get() ) );
	return 0;
}

// Every record checked on the device and the window bytes counted (n_hits > 0, hit_structures_args has passed): one
// synchronisation.  A call of one chunk leaves that chunk's spans in the scratch.
int hit_structures_count( rma_scanner_t *sc, const rma_db *db, const int32_t *d_hits, int64_t n_hits, void *stream, int64_t *total,
	char *err, size_t errlen )
{
	rma::HitPost	&p = *sc->post;
	rma::HitWindowScratch	*s = p.win;
	hipStream_t	st = s->stream.get();
	const int	stride = rma_hit_stride( &sc->prog );
	// HB_RECORD: the least index of a bad record, counted over the call; HB_STRUCT_SPARE: where the spans of a later
	// chunk, which count from the chunk's first record, put theirs (the same records, already judged).  A call of one
	// chunk has no pass over all records: the chunk's own spans judge them.
	const bool	chunks = n_hits > HW_CHUNK;
	if( check_records( s, db, sc->prog, d_hits, n_hits, stream, chunks, p.hs_carry(), sizeof( int64_t ), err, errlen ) )
		return 1;
	HIPCHK( rma::hit_helix_check( d_hits, n_hits, stride, p.hs_table(), s->d_bad + rma::HB_RECORD, st ) );
	for( int64_t c0 = 0; c0 < n_hits; c0 += HW_CHUNK ){
		const int64_t	cn = std::min( HW_CHUNK, n_hits - c0 );
		if( hit_structures_spans( sc, db, d_hits + c0 * stride, cn, s->d_bad + ( chunks ? rma::HB_STRUCT_SPARE : rma::HB_RECORD ), err, errlen ) )
			return 1;
		HIPCHK( rma::hit_carry_add( p.hs_carry(), s->d_off + cn, st ) );
	}
	HIPCHK( hipMemcpyAsync( s->h_bad + rma::HBH_FIRST, s->d_bad + rma::HB_RECORD, sizeof( unsigned long long ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipMemcpyAsync( s->h_bad + rma::HBH_TOTAL, p.hs_carry(), sizeof( int64_t ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipStreamSynchronize( st ) );
	if( s->h_bad[ rma::HBH_FIRST ] != ~0ull ){
		const rma::HitStructTable	tab = rma::hitstruct_table( sc->prog );
		return bad_record( s, db, sc->prog, d_hits, int64_t( s->h_bad[ rma::HBH_FIRST ] ), &tab, "written", err, errlen );
	}
	*total = int64_t( s->h_bad[ rma::HBH_TOTAL ] );
	return 0;
}

}	// namespace

extern "C" int rma_hit_structures_size( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
	void *stream, int64_t *total, char *err, size_t errlen )
{
	*total = 0;
	if( hit_structures_args( sc, db, d_hits, n_hits, "rma_hit_structures_size", err, errlen ) )
		return 1;
	return n_hits == 0 ? 0 : hit_structures_count( sc, db, d_hits, n_hits, stream, total, err, errlen );
}

extern "C" int rma_hit_structures( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
	const uint8_t *letters, int64_t total, int64_t *d_off, int32_t *d_lo, uint8_t *d_base, int16_t *d_elem, int32_t *d_mate,
	void *stream, char *err, size_t errlen )
{
	const char	*who = "rma_hit_structures";
	if( hit_structures_args( sc, db, d_hits, n_hits, who, err, errlen ) )
		return 1;
	if( total < 0 || total > INT64_MAX / 16 || d_off == nullptr || ( n_hits > 0 && d_lo == nullptr ) ||
		( total > 0 && ( d_base == nullptr || d_elem == nullptr || d_mate == nullptr ) ) ){
		snprintf( err, errlen, "%s: %lld window bytes: bad arguments", who, ( long long )total );
		return 1;
	}
	// the outputs: the caller's, each inside its allocation on the scanner's device
	if( rma::check_device_bytes( d_off, sc->device, 0, ( n_hits + 1 ) * 8, "the offsets", err, errlen ) ||
		( n_hits > 0 && rma::check_device_bytes( d_lo, sc->device, 0, n_hits * 4, "the first positions", err, errlen ) ) ||
		( total > 0 && ( rma::check_device_bytes( d_base, sc->device, 0, total, "the bases", err, errlen ) ||
			rma::check_device_bytes( d_elem, sc->device, 0, total * 2, "the elements", err, errlen ) ||
			rma::check_device_bytes( d_mate, sc->device, 0, total * 12, "the mates", err, errlen ) ) ) )
		return 1;
	hipStream_t	caller = static_cast<hipStream_t>( stream );
	int64_t	found = 0;
	const uint8_t	*tab = nullptr;
	int	codes = 0;
	// the letters as rma_replay_device takes them, on their way ahead of the count, whose synchronisation leaves the
	// page-locked copy free for the next call
	if( n_hits > 0 && ( letters_on_device( sc->post->win, db, letters, &tab, &codes, err, errlen ) ||
		hit_structures_count( sc, db, d_hits, n_hits, stream, &found, err, errlen ) ) )
		return 1;
	if( found != total ){
		snprintf( err, errlen, "%s: the windows of the %lld records have %lld bytes, not the %lld of `total`: nothing written", who,
			( long long )n_hits, ( long long )found, ( long long )total );
		return 1;
	}
	if( n_hits == 0 ){
		HIPCHK( hipMemsetAsync( d_off, 0, sizeof( int64_t ), caller ) );
		return 0;
	}
	rma::HitPost	&p = *sc->post;
	rma::HitWindowScratch	*s = p.win;
	hipStream_t	st = s->stream.get();
	const int	stride = rma_hit_stride( &sc->prog );
	HIPCHK( hipMemsetAsync( p.hs_carry(), 0, sizeof( int64_t ), st ) );
	for( int64_t c0 = 0; c0 < n_hits; c0 += HW_CHUNK ){
		const int64_t	cn = std::min( HW_CHUNK, n_hits - c0 );
		const int32_t	*ch = d_hits + c0 * stride;
		// (a call of one chunk: the count's spans are still there)
		if( n_hits > HW_CHUNK && hit_structures_spans( sc, db, ch, cn, s->d_bad + rma::HB_STRUCT_SPARE, err, errlen ) )
			return 1;
		const rma::HitStructOut	out{ d_off + c0, d_lo + c0, d_base, d_elem, d_mate };
		HIPCHK( rma::hit_struct_fill( db->text, ch, cn, stride, rma::hitwin_shape( sc->prog ), p.hs_table(), s->d_lo, s->d_src, s->d_off,
			p.hs_carry(), tab, codes, out, c0 + cn == n_hits, st ) );
		HIPCHK( rma::hit_carry_add( p.hs_carry(), s->d_off + cn, st ) );
	}
	return rma::stream_after( caller, st, err, errlen );
}

// ---------------------------------------------------------------- hit records as an alignment
// rma_hit_alignment_shape() / rma_hit_alignment(): the record check of rm_hitwin_dev.hip over all records, then the
// widths and fill kernels of rm_hitalign_dev.hip in chunks of HW_CHUNK records, on the stream of the scanner's span
// scratch, behind the caller's stream and, when something was written, ahead of what the caller queues next.  The
// call's 102 width words lie where that scratch keeps a chunk's window lengths, which neither kernel needs.
namespace {

// Every record checked on the device and the widths of the columns reduced over all of them into need[ HA_MAX_COLS ]
// (n_hits > 0, hit_structures_args has passed): one synchronisation.
int hit_alignment_widths( rma_scanner_t *sc, const rma_db *db, const int32_t *d_hits, int64_t n_hits, void *stream, int32_t *need,
	char *err, size_t errlen )
{
	rma::HitWindowScratch	*s = sc->post->win;
	hipStream_t	st = s->stream.get();
	const int	stride = rma_hit_stride( &sc->prog );
	const rma::HitWinShape	shape = rma::hitwin_shape( sc->prog );
	int32_t	*d_w = reinterpret_cast<int32_t *>( s->d_len ), *h_w = reinterpret_cast<int32_t *>( s->h_off );
	if( check_records( s, db, sc->prog, d_hits, n_hits, stream, true, d_w, rma::HA_MAX_COLS * sizeof( int32_t ), err, errlen ) )
		return 1;
	for( int64_t c0 = 0; c0 < n_hits; c0 += HW_CHUNK )
		HIPCHK( rma::hit_align_widths( d_hits + c0 * stride, std::min( HW_CHUNK, n_hits - c0 ), stride, shape, d_w, st ) );
	HIPCHK( hipMemcpyAsync( s->h_bad + rma::HBH_FIRST, s->d_bad + rma::HB_RECORD, sizeof( unsigned long long ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipMemcpyAsync( h_w, d_w, rma::HA_MAX_COLS * sizeof( int32_t ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipStreamSynchronize( st ) );
	if( s->h_bad[ rma::HBH_FIRST ] != ~0ull )
		return bad_record( s, db, sc->prog, d_hits, int64_t( s->h_bad[ rma::HBH_FIRST ] ), nullptr, "written", err, errlen );
	memcpy( need, h_w, rma::HA_MAX_COLS * sizeof( int32_t ) );
	return 0;
}

}	// namespace

extern "C" int rma_hit_alignment_shape( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
	int32_t *n_cols, int32_t *widths, uint8_t *right, int64_t *row_bytes, void *stream, char *err, size_t errlen )
{
	const char	*who = "rma_hit_alignment_shape";
	if( sc == nullptr || n_cols == nullptr || widths == nullptr || row_bytes == nullptr ){
		snprintf( err, errlen, "%s: no %s", who, sc == nullptr ? "scanner" : "room for the shape" );
		return 1;
	}
	if( hit_structures_args( sc, db, d_hits, n_hits, who, err, errlen ) )
		return 1;
	int32_t	need[ rma::HA_MAX_COLS ];
	memset( need, 0, sizeof( need ) );
	if( n_hits > 0 && hit_alignment_widths( sc, db, d_hits, n_hits, stream, need, err, errlen ) )
		return 1;
	const int	nc = rma::hitalign_n_cols( rma::hitwin_shape( sc->prog ) );
	*n_cols = nc;
	if( right != nullptr )
		rma::hitalign_directions( sc->prog, right );
	int64_t	w = nc - 1;
	for( int c = 0; c < rma::HA_MAX_COLS; c++ ){
		widths[ c ] = c < nc ? need[ c ] : 0;
		w += widths[ c ];
	}
	*row_bytes = w;
	return 0;
}

extern "C" int rma_hit_alignment( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
	const int32_t *widths, const uint8_t *letters, const uint8_t *fill, uint8_t *d_rows, int32_t *d_pos,
	void *stream, char *err, size_t errlen )
{
	const char	*who = "rma_hit_alignment";
	if( sc == nullptr || widths == nullptr ){
		snprintf( err, errlen, "%s: no %s", who, sc == nullptr ? "scanner" : "widths" );
		return 1;
	}
	if( hit_structures_args( sc, db, d_hits, n_hits, who, err, errlen ) )
		return 1;
	const int	nc = rma::hitalign_n_cols( rma::hitwin_shape( sc->prog ) );
	for( int c = 0; c < nc; c++ )
		if( widths[ c ] < 0 ){
			snprintf( err, errlen, "%s: column %d: width %d: nothing written", who, c, widths[ c ] );
			return 1;
		}
	static const uint8_t	tool_fill[ 3 ] = { '-', '|', '.' };
	const rma::HitAlignLayout	lay = rma::hitalign_layout( sc->prog, widths, fill != nullptr ? fill : tool_fill );
	const int64_t	W = lay.row_bytes;
	if( n_hits == 0 )
		return 0;
	if( d_rows == nullptr || W > INT64_MAX / 16 / n_hits ){
		snprintf( err, errlen, "%s: %lld rows of %lld bytes: bad arguments", who, ( long long )n_hits, ( long long )W );
		return 1;
	}
	// the outputs: the caller's, each inside its allocation on the scanner's device
	if( W > 0 && ( rma::check_device_bytes( d_rows, sc->device, 0, n_hits * W, "the rows", err, errlen ) ||
		( d_pos != nullptr && rma::check_device_bytes( d_pos, sc->device, 0, n_hits * W * 4, "the positions", err, errlen ) ) ) )
		return 1;
	rma::HitWindowScratch	*s = sc->post->win;
	hipStream_t	st = s->stream.get(), caller = static_cast<hipStream_t>( stream );
	// the letters, as rma_hit_structures takes them: on their way ahead of the check, whose synchronisation leaves the
	// page-locked copy free for the next call
	const uint8_t	*tab = nullptr;
	int	codes = 0;
	if( letters_on_device( s, db, letters, &tab, &codes, err, errlen ) )
		return 1;
	int32_t	need[ rma::HA_MAX_COLS ];
	if( hit_alignment_widths( sc, db, d_hits, n_hits, stream, need, err, errlen ) )
		return 1;
	for( int c = 0; c < nc; c++ )
		if( widths[ c ] < need[ c ] ){
			snprintf( err, errlen, "%s: column %d: width %d given, the records need %d: nothing written", who, c, widths[ c ], need[ c ] );
			return 1;
		}
	const int	stride = rma_hit_stride( &sc->prog );
	for( int64_t c0 = 0; c0 < n_hits; c0 += HW_CHUNK )
		HIPCHK( rma::hit_align_fill( db->text, d_hits + c0 * stride, std::min( HW_CHUNK, n_hits - c0 ), stride, rma::hitwin_shape( sc->prog ), lay,
			db->d_slen, db->d_text_start, tab, codes, d_rows + c0 * W, d_pos != nullptr ? d_pos + c0 * W : nullptr, st ) );
	return rma::stream_after( caller, st, err, errlen );
}

// ---------------------------------------------------------------- rmprune's rule over records on the device
// rma_prune_hits(): the kernels of rm_prune_dev.hip on the caller's stream.  The scratch -- the program's table, a
// call's keys, flags and list of blocks, the entries' name groups -- is the scanner's, made on the first call and
// grown; a later call on another stream waits for the kernels of the one before it (pr_done).  One wait, for two
// words: the least index of a refused record and the number of blocks, which sizes the last launch.  The database
// may be any: only its entry lengths are read.
extern "C" int rma_prune_hits( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
	const int32_t *group_of_entry, uint8_t *d_keep, void *stream, char *err, size_t errlen )
{
	const char	*who = "rma_prune_hits";
	if( sc == nullptr || db == nullptr ){
		snprintf( err, errlen, "%s: no %s", who, sc == nullptr ? "scanner" : "database" );
		return 1;
	}
	const int	stride = rma_hit_stride( &sc->prog );
	const rma::PruneTable	tab = rma::prune_table( sc->prog );
	const int	row = rma::prune_row_words( tab );
	// (n_hits * 16 bytes of headers, n_hits * row * 4 of key rows, n_hits * stride * 4 of records; records without
	// flags to write are refused as records without records)
	const RecordCall	call{ who, sc->device, false, INT64_MAX / 16 / std::max( stride, row ) };
	if( record_call_args( call, db, stride, d_keep != nullptr ? d_hits : nullptr, n_hits, err, errlen ) )
		return 1;
	if( n_hits == 0 )
		return 0;
	if( rma::check_device_bytes( d_keep, sc->device, 0, n_hits, "the keep flags", err, errlen ) )
		return 1;
	rma::HitPost	&p = post_of( sc );
	hipStream_t	st = static_cast<hipStream_t>( stream );
	if( !p.pr_table ){
		rma::DevMem	table;
		rma::PinMem	words;
		rma::Event	done;
		HIPCHK( table.exact( align256( sizeof( rma::PruneTable ) ) + 256 ) );
		HIPCHK( hipMemcpy( table.as<void>(), &tab, sizeof( tab ), hipMemcpyHostToDevice ) );
		HIPCHK( words.exact( 256 ) );
		HIPCHK( done.create( hipEventDisableTiming ) );
		HIPCHK( hipEventRecord( done.get(), st ) );
		p.pr_table = std::move( table );
		p.h_pr = std::move( words );
		p.pr_done = std::move( done );
	}
	// behind the kernels of the call before this one (they read the scratch) and the database's tables
	HIPCHK( hipStreamWaitEvent( st, p.pr_done.get(), 0 ) );
	HIPCHK( hipStreamWaitEvent( st, db->ready.get(), 0 ) );
	const size_t	n = size_t( n_hits ), parts = size_t( rma::prune_parts( n_hits ) );
	rma::PruneDev	pd;
	HIPCHK( p.d_pr.room( rma::prune_carve( pd, nullptr, n, parts, size_t( row ) ) ) );
	rma::prune_carve( pd, p.d_pr.as<void>(), n, parts, size_t( row ) );
	char	*dt = p.pr_table.as<char>() + align256( sizeof( rma::PruneTable ) );
	pd.tab = p.pr_table.as<rma::PruneTable>();
	pd.groups = nullptr;
	pd.bad = reinterpret_cast<unsigned long long *>( dt );
	pd.n_blocks = reinterpret_cast<long long *>( dt + 8 );
	if( group_of_entry != nullptr && db->n_seq > 0 ){
		// (pageable memory: the copy has left the caller's array when the call returns)
		HIPCHK( p.d_pr_groups.room( size_t( db->n_seq ) * 4 ) );
		HIPCHK( hipMemcpyAsync( p.d_pr_groups.as<void>(), group_of_entry, size_t( db->n_seq ) * 4, hipMemcpyHostToDevice, st ) );
		pd.groups = p.d_pr_groups.as<int32_t>();
	}
	HIPCHK( hipMemsetAsync( pd.bad, 0xff, sizeof( unsigned long long ), st ) );
	HIPCHK( hipMemsetAsync( pd.n_blocks, 0, sizeof( long long ), st ) );
	HIPCHK( rma::prune_blocks( d_hits, n_hits, stride, rma::hitwin_shape( sc->prog ), row, db->d_slen, db->n_seq, pd, st ) );
	unsigned long long	*h = p.h_pr.as<unsigned long long>();
	HIPCHK( hipMemcpyAsync( h, pd.bad, 16, hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipStreamSynchronize( st ) );
	if( h[ 0 ] != ~0ull ){
		if( scratch_on( &p.win, sc->device, err, errlen ) )
			return 1;
		return bad_record( p.win, db, sc->prog, d_hits, int64_t( h[ 0 ] ), nullptr, "judged", err, errlen );
	}
	const int64_t	n_blocks = int64_t( h[ 1 ] );
	if( n_blocks < 1 || n_blocks > n_hits ){
		snprintf( err, errlen, "%s: %lld blocks of %lld records (records changed during the call?)", who, ( long long )n_blocks, ( long long )n_hits );
		return 1;
	}
	HIPCHK( rma::prune_rezip( n_hits, row, pd, n_blocks, d_keep, st ) );
	HIPCHK( hipEventRecord( p.pr_done.get(), st ) );
	return 0;
}

// ---------------------------------------------------------------- energies of structures in device tensors
// rma_scanner_load_energy_tables(): efn's and efn2's tables from a directory onto the scanner's device, where
// rma_scanner_create() and rma_scanner_set_efn2data() put a descriptor's.  No scan changes: the scan's energy kernel is
// launched for a descriptor's call sites only (rm_scanner.cpp launch_efn), and a descriptor with call sites has its
// tables from the start; tables loaded again replace the ones that are there.
extern "C" int rma_scanner_load_energy_tables( rma_scanner_t *sc, const char *dir, int which, char *err, size_t errlen )
{
	const char	*who = "rma_scanner_load_energy_tables";
	if( sc == nullptr || which < 1 || which > 3 ){
		snprintf( err, errlen, "%s: %s", who, sc == nullptr ? "no scanner" : "which: 1 (efn), 2 (efn2) or 3 (both)" );
		return 1;
	}
	if( sc->fly.db != nullptr ){
		snprintf( err, errlen, "%s: a scan is in flight (rma_scan_begin without rma_scan_end): its energy kernel reads the tables", who );
		return 1;
	}
	// (read first: a directory without the files leaves the scanner as it was)
	std::unique_ptr<rma_efndata_t>	efn;
	std::unique_ptr<rma_efn2data_t>	efn2;
	if( which & 1 ){
		efn.reset( new rma_efndata_t );
		if( rma_efndata_load( dir, efn.get(), err, errlen ) )
			return 1;
	}
	if( which & 2 ){
		efn2.reset( new rma_efn2data_t );
		if( rma_efn2data_load( dir, efn2.get(), err, errlen ) )
			return 1;
	}
	HIPCHK( hipSetDevice( sc->device ) );
	// (behind the energy kernels of rma_structure_energies calls that read the tables now)
	if( sc->post != nullptr && sc->post->se_done.get() != nullptr )
		HIPCHK( hipEventSynchronize( sc->post->se_done.get() ) );
	if( efn && rma::efn_tables_to_device( sc, efn.get(), err, errlen ) )
		return 1;
	if( efn2 && rma_scanner_set_efn2data( sc, efn2.get(), err, errlen ) )
		return 1;
	return 0;
}

namespace {

constexpr size_t	SE_CODES_AT = 256;		// the codes behind the two result words, in both fixed blocks

// the words of a refusal: structure s judged again on the host, by the rule the kernel applied (rm_structenergy.h)
int bad_structure( const rma::StructBatch &b, int64_t s, hipStream_t st, char *err, size_t errlen )
{
	const char	*who = "rma_structure_energies";
	int64_t	o[ 2 ];
	HIPCHK( hipMemcpyAsync( o, b.off + s, sizeof( o ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipStreamSynchronize( st ) );
	const long long	lo = o[ 0 ], hi = o[ 1 ], ls = s;
	const char	*nothing = "nothing written";
	switch( rmse_check_offsets( lo, hi, s, b.n, b.total ) ){
	case RMSE_OK :
		break;
	case RMSE_OFF_FIRST :
		snprintf( err, errlen, "%s: structure %lld: off[ 0 ] is %lld, not 0: %s", who, ls, lo, nothing );
		return 1;
	case RMSE_OFF_DECREASES :
		snprintf( err, errlen, "%s: structure %lld: off decreases from %lld to %lld: %s", who, ls, lo, hi, nothing );
		return 1;
	case RMSE_OFF_OUTSIDE :
		snprintf( err, errlen, "%s: structure %lld: bases [%lld, %lld) outside the %lld of `total`: %s", who, ls, lo, hi, ( long long )b.total, nothing );
		return 1;
	case RMSE_OFF_LAST :
		snprintf( err, errlen, "%s: structure %lld: off[ n ] is %lld, not the %lld of `total`: %s", who, ls, hi, ( long long )b.total, nothing );
		return 1;
	default :
		snprintf( err, errlen, "%s: structure %lld: %lld bases, more than %d: %s", who, ls, hi - lo, RMSE_MAX_BASES, nothing );
		return 1;
	}
	const int	len = int( hi - lo );
	std::vector<int32_t>	pair( size_t( std::max( len, 1 ) ) );
	if( len > 0 ){
		HIPCHK( hipMemcpy2DAsync( pair.data(), 4, b.pair + lo * b.pair_stride, size_t( b.pair_stride ) * 4, 4, size_t( len ), hipMemcpyDeviceToHost, st ) );
		HIPCHK( hipStreamSynchronize( st ) );
	}
	const rmse_pairs_t	view{ pair.data(), 1 };
	int	which = 0, info = 0;
	switch( rmse_check_structure( view, len, &which, &info ) ){
	case RMSE_PAIR_RANGE :
		snprintf( err, errlen, "%s: structure %lld: base %d pairs with %d, outside its %d bases: %s", who, ls, which, pair[ size_t( which ) ], len, nothing );
		return 1;
	case RMSE_PAIR_SELF :
		snprintf( err, errlen, "%s: structure %lld: base %d pairs with itself: %s", who, ls, which, nothing );
		return 1;
	case RMSE_PAIR_ASYM :
		snprintf( err, errlen, "%s: structure %lld: base %d pairs with %d, which pairs with %d: %s", who, ls, which, pair[ size_t( which ) ],
			pair[ size_t( pair[ size_t( which ) ] ) ], nothing );
		return 1;
	case RMSE_HELICES :
		snprintf( err, errlen, "%s: structure %lld: %d helices, more than %d: %s", who, ls, which, RMSE_MAX_HELICES, nothing );
		return 1;
	default :
		snprintf( err, errlen, "%s: structure %lld: refused on the device, not on the host (tensors changed during the call?)", who, ls );
		return 1;
	}
}

}	// namespace

// rma_structure_energies(): the kernels of rm_structenergy_dev.hip on the caller's stream -- the check of every
// structure, one wait for its two words (the least index of a refused structure, whether some structure needs the
// large stacks), then the energy kernel's one or two instances, for which the call does not wait.  The scratch -- the
// two words, the codes of the call's bytes, an info word per structure -- is the scanner's, made on the first call and
// grown; a later call on another stream waits for the kernels of the one before it (se_done).
extern "C" int rma_structure_energies( rma_scanner_t *sc, const int64_t *d_off, const uint8_t *d_base, const int32_t *d_pair,
	int32_t pair_stride, int64_t n, int64_t total, const uint8_t *letters, int32_t *d_efn, int32_t *d_efn2, void *stream,
	char *err, size_t errlen )
{
	const char	*who = "rma_structure_energies";
	if( sc == nullptr ){
		snprintf( err, errlen, "%s: no scanner", who );
		return 1;
	}
	// (( n + 1 ) * 8 bytes of offsets, total * pair_stride * 4 of partners)
	if( n < 0 || total < 0 || pair_stride < 1 || n > INT64_MAX / 16 || total > INT64_MAX / 16 / pair_stride ||
		( n > 0 && d_off == nullptr ) || ( n > 0 && total > 0 && ( d_base == nullptr || d_pair == nullptr ) ) ){
		snprintf( err, errlen, "%s: %lld structures of %lld bases, partners every %d words: bad arguments", who, ( long long )n,
			( long long )total, pair_stride );
		return 1;
	}
	if( n == 0 )
		return 0;
	if( ( d_efn != nullptr && !sc->have_efn ) || ( d_efn2 != nullptr && !sc->d_efn2 ) ){
		snprintf( err, errlen, "%s: the scanner has no %s tables: its descriptor has no such call, and rma_scanner_load_energy_tables() was not called",
			who, d_efn != nullptr && !sc->have_efn ? "efn()" : "efn2()" );
		return 1;
	}
	HIPCHK( hipSetDevice( sc->device ) );
	if( rma::check_device_bytes( d_off, sc->device, 0, ( n + 1 ) * 8, "the offsets", err, errlen ) ||
		( total > 0 && ( rma::check_device_bytes( d_base, sc->device, 0, total, "the bases", err, errlen ) ||
			rma::check_device_bytes( d_pair, sc->device, 0, ( ( total - 1 ) * pair_stride + 1 ) * 4, "the partners", err, errlen ) ) ) ||
		( d_efn != nullptr && rma::check_device_bytes( d_efn, sc->device, 0, n * 4, "the efn energies", err, errlen ) ) ||
		( d_efn2 != nullptr && rma::check_device_bytes( d_efn2, sc->device, 0, n * 4, "the efn2 energies", err, errlen ) ) )
		return 1;
	rma::HitPost	&p = post_of( sc );
	hipStream_t	st = static_cast<hipStream_t>( stream );
	if( !p.d_se ){
		rma::DevMem	dev;
		rma::PinMem	pin;
		rma::Event	done;
		HIPCHK( dev.exact( SE_CODES_AT + 256 ) );
		HIPCHK( pin.exact( SE_CODES_AT + 256 ) );
		HIPCHK( done.create( hipEventDisableTiming ) );
		HIPCHK( hipEventRecord( done.get(), st ) );
		p.d_se = std::move( dev );
		p.h_se = std::move( pin );
		p.se_done = std::move( done );
	}
	// behind the kernels of the call before this one: they read the scratch
	HIPCHK( hipStreamWaitEvent( st, p.se_done.get(), 0 ) );
	HIPCHK( p.d_se_info.room( size_t( n ) * 4 ) );
	unsigned long long	*d_bad = p.d_se.as<unsigned long long>(), *h_bad = p.h_se.as<unsigned long long>();
	uint8_t	*d_code = p.d_se.as<uint8_t>() + SE_CODES_AT, *h_code = p.h_se.as<uint8_t>() + SE_CODES_AT;
	// (the page-locked copy is free: every call before this one has waited behind its upload)
	for( int b = 0; b < 256; b++ )
		h_code[ b ] = uint8_t( rmse_letter_code( letters != nullptr ? letters[ b ] : rma::hitwin_reader_letter( static_cast<unsigned char>( b ) ) ) );
	HIPCHK( hipMemcpyAsync( d_code, h_code, 256, hipMemcpyHostToDevice, st ) );
	HIPCHK( hipMemsetAsync( d_bad, 0xff, sizeof( unsigned long long ), st ) );
	HIPCHK( hipMemsetAsync( d_bad + 1, 0, sizeof( unsigned long long ), st ) );
	const rma::StructBatch	batch{ d_off, d_base, d_pair, pair_stride, n, total };
	int32_t	*d_info = p.d_se_info.as<int32_t>();
	const int	cus = sc->grid_blocks / 8, wgs = sc->opt.struct_wgs;
	HIPCHK( rma::struct_check( batch, d_info, d_bad, wgs, cus, st ) );
	HIPCHK( hipMemcpyAsync( h_bad, d_bad, 2 * sizeof( unsigned long long ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipStreamSynchronize( st ) );
	if( h_bad[ 0 ] != ~0ull )
		return bad_structure( batch, int64_t( h_bad[ 0 ] ), st, err, errlen );
	if( d_efn != nullptr || d_efn2 != nullptr ){
		const rma::StructTables	t{ d_efn != nullptr ? sc->d_t16.as<int16_t>() : nullptr, sc->d_tlkey.as<int32_t>(), sc->d_loginc.as<int32_t>(),
			d_efn2 != nullptr ? sc->efn2() : nullptr, d_code };
		HIPCHK( rma::struct_energies( batch, d_info, t, d_efn, d_efn2, 0, wgs, cus, st ) );
		if( h_bad[ 1 ] != 0 )
			HIPCHK( rma::struct_energies( batch, d_info, t, d_efn, d_efn2, 1, wgs, cus, st ) );
	}
	HIPCHK( hipEventRecord( p.se_done.get(), st ) );
	return 0;
}

// ---------------------------------------------------------------- the score section over records on the device
// rma_score_hits(): rma_score_kernel (rm_score_dev.hip) in chunks of HW_CHUNK records on the stream of the scanner's span
// scratch, behind the caller's stream.  The kernel checks each record by the span rule before it runs MAIN on it, so
// the call has no pass of its own for the check.  Results go to scratch of the scanner's; one wait learns the least
// index of a bad and of a stopped record; then the results are copied to the caller's tensors, ahead of what the caller
// queues next.  For a stopped record the kernel runs once more, on that record alone, to fetch the stop's particulars.
namespace {
constexpr size_t	SC_DETAIL_AT = 64, SC_RESULTS_AT = 256;
}

// rma_score_hits_text() is the same call with three more outputs: the score column of every record as bytes, in scratch
// like the rest, copied out row by row up to each row's length.  An image with RMS_IMG_TEXT brings its table of bits()
// behind its bytes and takes a chunk's heaps from the scanner; it and every text call run rma_score_text_kernel.
static int score_hits( const char *who, bool text_call, rma_scanner_t *sc, const rma_score_t *sp, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
	const uint8_t *letters, uint8_t *d_accept, double *d_score, int8_t *d_kind, uint8_t *d_text, int32_t text_stride, int32_t *d_text_len,
	void *stream, char *err, size_t errlen )
{
	if( sc == nullptr || sp == nullptr || db == nullptr ){
		snprintf( err, errlen, "%s: no %s", who, sc == nullptr ? "scanner" : sp == nullptr ? "score program" : "database" );
		return 1;
	}
	// (both are memcpy copies of a descriptor's program: padding bytes included, equal where the descriptor's are)
	if( memcmp( sp->img.prog.get(), &sc->prog, sizeof( rma_program_t ) ) != 0 ){
		snprintf( err, errlen, "%s: the score program was opened for another descriptor than the scanner's (their programs differ): nothing written", who );
		return 1;
	}
	if( hit_structures_args( sc, db, d_hits, n_hits, who, err, errlen ) )
		return 1;
	if( n_hits == 0 )
		return 0;
	if( d_accept == nullptr || ( text_call && ( d_text == nullptr || d_text_len == nullptr ) ) ){
		snprintf( err, errlen, "%s: %lld records: bad arguments", who, ( long long )n_hits );
		return 1;
	}
	if( text_call && ( text_stride < 1 || n_hits > ( int64_t( 1 ) << 40 ) / text_stride ) ){
		snprintf( err, errlen, "%s: %lld records, rows of %d bytes: bad arguments", who, ( long long )n_hits, text_stride );
		return 1;
	}
	if( text_call && ( rma::check_device_bytes( d_text, sc->device, 0, n_hits * text_stride, "the text", err, errlen ) ||
		rma::check_device_bytes( d_text_len, sc->device, 0, n_hits * 4, "the text's lengths", err, errlen ) ) )
		return 1;
	if( rma::check_device_bytes( d_accept, sc->device, 0, n_hits, "the accept flags", err, errlen ) ||
		( d_score != nullptr && rma::check_device_bytes( d_score, sc->device, 0, n_hits * 8, "the scores", err, errlen ) ) ||
		( d_kind != nullptr && rma::check_device_bytes( d_kind, sc->device, 0, n_hits, "the kinds", err, errlen ) ) )
		return 1;
	if( letters != nullptr )
		for( int b = 0; b < 256; b++ )
			if( letters[ b ] == 0 ){
				snprintf( err, errlen, "%s: the letters give byte %d the letter 0, which ends a string of the score section: nothing written", who, b );
				return 1;
			}
	const RmsImage	*m = sp->img.image();
	const int	frames = rms_frames( m );	// (>= 0: an image with expressions, which runs the match kernels)
	if( rma::score_waves( m->bytes, m->stack, m->n_vars, frames ) < 1 ){
		snprintf( err, errlen, "%s: the image leaves no room for a wave", who );
		return 1;
	}
	rma::HitPost	&p = *sc->post;
	rma::HitWindowScratch	*s = p.win;
	hipStream_t	st = s->stream.get(), caller = static_cast<hipStream_t>( stream );
	const bool	img_text = ( m->flags & RMS_IMG_TEXT ) != 0, text_kernel = text_call || img_text;
	const size_t	n = size_t( n_hits ), flags = ( n + 7 ) & ~size_t( 7 ), rows = text_call ? ( n * size_t( text_stride ) + 7 ) & ~size_t( 7 ) : 0;
	const size_t	want = SC_RESULTS_AT + 2 * flags + 8 * n + rows + ( text_call ? 4 * n : 0 );
	const int	heap_cap = img_text ? sc->opt.score_heap : 0;
	const size_t	heap = rma::score_heap_bytes( ( long long )std::min( HW_CHUNK, n_hits ), heap_cap );
	if( heap > p.d_sc_heap.bytes() ){
		HIPCHK( hipStreamSynchronize( st ) );
		HIPCHK( p.d_sc_heap.room( heap ) );
	}
	if( want > p.d_sc.bytes() )		// (the copies of the call before this one may still read the block that goes)
		HIPCHK( hipStreamSynchronize( st ) );
	HIPCHK( p.d_sc.room( want ) );
	if( !p.h_sc )
		HIPCHK( p.h_sc.exact( SC_RESULTS_AT ) );
	if( p.sc_serial != sp->img.serial ){
		HIPCHK( hipStreamSynchronize( st ) );
		p.sc_serial = 0;		// (no image's until this one's bytes are in)
		const size_t	table = sp->img.bits_tab.size() * sizeof( double );
		HIPCHK( p.d_sc_image.room( size_t( m->bytes ) + table ) );
		HIPCHK( hipMemcpy( p.d_sc_image.as<void>(), m, size_t( m->bytes ), hipMemcpyHostToDevice ) );
		if( table > 0 )
			HIPCHK( hipMemcpy( p.d_sc_image.as<char>() + m->bytes, sp->img.bits_tab.data(), table, hipMemcpyHostToDevice ) );
		p.sc_serial = sp->img.serial;
	}
	const uint8_t	*tab = nullptr;
	int	codes = 0;
	if( letters_on_device( s, db, letters, &tab, &codes, err, errlen ) ||
		check_records( s, db, sc->prog, d_hits, n_hits, stream, false, nullptr, 0, err, errlen ) )
		return 1;
	char	*base = p.d_sc.as<char>();
	unsigned long long	*d_words = reinterpret_cast<unsigned long long *>( base ), *h_words = p.h_sc.as<unsigned long long>();
	RmsResult	*d_detail = reinterpret_cast<RmsResult *>( base + SC_DETAIL_AT );
	RmsResult	*h_detail = reinterpret_cast<RmsResult *>( p.h_sc.as<char>() + SC_DETAIL_AT );
	uint8_t	*acc = reinterpret_cast<uint8_t *>( base + SC_RESULTS_AT );
	int8_t	*kind = reinterpret_cast<int8_t *>( acc + flags );
	double	*score = reinterpret_cast<double *>( acc + 2 * flags );
	uint8_t	*text = reinterpret_cast<uint8_t *>( score + n );
	int32_t	*text_len = reinterpret_cast<int32_t *>( text + rows );
	const double	*bits_tab = sp->img.bits_tab.empty() ? nullptr : reinterpret_cast<const double *>( p.d_sc_image.as<char>() + m->bytes );
	HIPCHK( hipMemsetAsync( d_words, 0xff, 2 * sizeof( unsigned long long ), st ) );
	const int	stride = rma_hit_stride( &sc->prog );
	auto batch = [&]( int64_t c0, int64_t cn, RmsResult *detail ){
		rma::ScoreBatch	b{ p.d_sc_image.as<RmsImage>(), m->bytes, m->stack, m->n_vars, d_hits + c0 * stride, ( long long )cn, ( long long )c0, stride,
			rma::hitwin_shape( sc->prog ), db->d_slen, db->d_text_start, db->n_seq, db->text, tab, codes, sc->opt.score_budget,
			acc + c0, score + c0, kind + c0, d_words, d_words + 1, detail };
		if( text_kernel ){
			b.text_kernel = 1;
			b.heap = heap > 0 ? p.d_sc_heap.as<uint8_t>() : nullptr;
			b.heap_cap = heap_cap;
			b.bits_tab = bits_tab;
			if( text_call ){
				b.col = text + c0 * text_stride;
				b.col_stride = text_stride;
				b.col_len = text_len + c0;
			}
		}
		if( frames >= 0 ){
			b.match_kernel = 1;
			b.frames = frames;
		}
		return b;
	};
	for( int64_t c0 = 0; c0 < n_hits; c0 += HW_CHUNK )
		HIPCHK( rma::score_records( batch( c0, std::min( HW_CHUNK, n_hits - c0 ), nullptr ), st ) );
	HIPCHK( hipMemcpyAsync( h_words, d_words, 2 * sizeof( unsigned long long ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipStreamSynchronize( st ) );
	if( h_words[ 0 ] != ~0ull )
		return bad_record( s, db, sc->prog, d_hits, int64_t( h_words[ 0 ] ), nullptr, "scored", err, errlen );
	if( h_words[ 1 ] != ~0ull ){
		const int64_t	h = int64_t( h_words[ 1 ] );
		memset( h_detail, 0, sizeof( RmsResult ) );
		HIPCHK( hipMemsetAsync( d_detail, 0, sizeof( RmsResult ), st ) );
		HIPCHK( rma::score_records( batch( h, 1, d_detail ), st ) );
		HIPCHK( hipMemcpyAsync( h_detail, d_detail, sizeof( RmsResult ), hipMemcpyDeviceToHost, st ) );
		HIPCHK( hipStreamSynchronize( st ) );
		snprintf( err, errlen, "%s: record %lld: %s: nothing written", who, ( long long )h, rma::score_stop_text( sp->img, *h_detail ).c_str() );
		return 1;
	}
	HIPCHK( hipMemcpyAsync( d_accept, acc, n, hipMemcpyDeviceToDevice, st ) );
	if( d_score != nullptr )
		HIPCHK( hipMemcpyAsync( d_score, score, 8 * n, hipMemcpyDeviceToDevice, st ) );
	if( d_kind != nullptr )
		HIPCHK( hipMemcpyAsync( d_kind, kind, n, hipMemcpyDeviceToDevice, st ) );
	if( text_call ){
		HIPCHK( rma::score_text_copy( d_text, text, text_len, ( long long )n_hits, text_stride, st ) );
		HIPCHK( hipMemcpyAsync( d_text_len, text_len, 4 * n, hipMemcpyDeviceToDevice, st ) );
	}
	return rma::stream_after( caller, st, err, errlen );
}

extern "C" int rma_score_hits( rma_scanner_t *sc, const rma_score_t *sp, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
	const uint8_t *letters, uint8_t *d_accept, double *d_score, int8_t *d_kind, void *stream, char *err, size_t errlen )
{
	return score_hits( "rma_score_hits", false, sc, sp, db, d_hits, n_hits, letters, d_accept, d_score, d_kind, nullptr, 0, nullptr, stream, err, errlen );
}

extern "C" int rma_score_hits_text( rma_scanner_t *sc, const rma_score_t *sp, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
	const uint8_t *letters, uint8_t *d_accept, double *d_score, int8_t *d_kind, uint8_t *d_text, int32_t text_stride, int32_t *d_text_len,
	void *stream, char *err, size_t errlen )
{
	return score_hits( "rma_score_hits_text", true, sc, sp, db, d_hits, n_hits, letters, d_accept, d_score, d_kind, d_text, text_stride, d_text_len,
		stream, err, errlen );
}

extern "C" void rma_score_info( const rma_score_t *sp, int32_t info[ 10 ] )
{
	if( sp == nullptr ){
		for( int i = 0; i < 10; i++ )
			info[ i ] = -1;
		return;
	}
	const RmsImage	*m = sp->img.image();
	const int	frames = rms_frames( m );
	const int	waves = rma::score_waves( m->bytes, m->stack, m->n_vars, frames ), wave = rms_wave_bytes( m->stack, m->n_vars, frames );
	info[ 0 ] = m->bytes;
	info[ 1 ] = m->n_inst;
	info[ 2 ] = m->n_vars;
	info[ 3 ] = m->stack;
	info[ 4 ] = wave;
	info[ 5 ] = waves;
	info[ 6 ] = m->bytes + RMS_LDS_TABLES + waves * wave;
	int	priv = -1, lds = -1, regs = -1;
	if( rma::score_kernel_attributes( &priv, &lds, &regs, ( m->flags & RMS_IMG_TEXT ) != 0, frames >= 0 ) != hipSuccess )
		( void )hipGetLastError();
	info[ 7 ] = priv;
	info[ 8 ] = lds;
	info[ 9 ] = regs;
}

// ---------------------------------------------------------------- loose seq= expressions over records on the device
// rma_seqcheck_hits(): rma_seqcheck_kernel (rm_seqcheck_dev.hip) in chunks of HW_CHUNK records on the stream of the
// scanner's span scratch, behind the caller's stream, as rma_score_hits runs its kernel: the kernel checks each record
// by the span rule before it applies the expressions to it; results go to scratch of the scanner's; one wait learns the
// least index of a bad and of a stopped record; then the results are copied to the caller's tensors, ahead of what the
// caller queues next.  For a stopped record the kernel runs once more, on that record alone, to learn its element.
namespace {
constexpr size_t	SQ_DETAIL_AT = 64, SQ_RESULTS_AT = 256;
}

extern "C" int rma_seqcheck_hits( rma_scanner_t *sc, const rma_seqcheck_t *sq, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
	const uint8_t *letters, int32_t budget, uint8_t *d_keep, int32_t *d_fixed, void *stream, char *err, size_t errlen )
{
	const char	*who = "rma_seqcheck_hits";
	if( sc == nullptr || sq == nullptr || db == nullptr ){
		snprintf( err, errlen, "%s: no %s", who, sc == nullptr ? "scanner" : sq == nullptr ? "seq= check" : "database" );
		return 1;
	}
	// (both are memcpy copies of a descriptor's program: padding bytes included, equal where the descriptor's are)
	if( memcmp( sq->img.prog.get(), &sc->prog, sizeof( rma_program_t ) ) != 0 ){
		snprintf( err, errlen, "%s: the seq= check was opened for another descriptor than the scanner's (their programs differ): nothing written", who );
		return 1;
	}
	if( budget < 0 ){
		snprintf( err, errlen, "%s: a budget of %d steps: bad arguments", who, budget );
		return 1;
	}
	if( budget == 0 )
		budget = RMQ_DEFAULT_BUDGET;
	if( hit_structures_args( sc, db, d_hits, n_hits, who, err, errlen ) )
		return 1;
	if( n_hits == 0 )
		return 0;
	if( d_keep == nullptr ){
		snprintf( err, errlen, "%s: %lld records: bad arguments", who, ( long long )n_hits );
		return 1;
	}
	const int	stride = rma_hit_stride( &sc->prog );
	const int64_t	row_bytes = n_hits * stride * 4;
	if( rma::check_device_bytes( d_keep, sc->device, 0, n_hits, "the keep flags", err, errlen ) ||
		( d_fixed != nullptr && rma::check_device_bytes( d_fixed, sc->device, 0, row_bytes, "the fixed rows", err, errlen ) ) )
		return 1;
	if( d_fixed != nullptr ){
		const char	*a = reinterpret_cast<const char *>( d_hits ), *f = reinterpret_cast<const char *>( d_fixed );
		if( a < f + row_bytes && f < a + row_bytes ){
			snprintf( err, errlen, "%s: the fixed rows overlap the records: nothing written", who );
			return 1;
		}
	}
	if( letters != nullptr )
		for( int b = 0; b < 256; b++ )
			if( letters[ b ] == 0 ){
				snprintf( err, errlen, "%s: the letters give byte %d the letter 0, which ends the text of an element: nothing written", who, b );
				return 1;
			}
	const RmqImage	*m = sq->img.image();
	if( rma::seqcheck_waves( m->bytes, m->frames ) < 1 || m->stride != stride ){
		snprintf( err, errlen, "%s: the image leaves no room for a wave", who );
		return 1;
	}
	rma::HitPost	&p = *sc->post;
	rma::HitWindowScratch	*s = p.win;
	hipStream_t	st = s->stream.get(), caller = static_cast<hipStream_t>( stream );
	const size_t	n = size_t( n_hits ), flags = ( n + 7 ) & ~size_t( 7 ), want = SQ_RESULTS_AT + flags + ( d_fixed != nullptr ? size_t( row_bytes ) : 0 );
	if( want > p.d_sq.bytes() )		// (the copies of the call before this one may still read the block that goes)
		HIPCHK( hipStreamSynchronize( st ) );
	HIPCHK( p.d_sq.room( want ) );
	if( !p.h_sq )
		HIPCHK( p.h_sq.exact( SQ_RESULTS_AT ) );
	if( p.sq_serial != sq->img.serial ){
		HIPCHK( hipStreamSynchronize( st ) );
		p.sq_serial = 0;		// (no image's until this one's bytes are in)
		HIPCHK( p.d_sq_image.room( size_t( m->bytes ) ) );
		HIPCHK( hipMemcpy( p.d_sq_image.as<void>(), m, size_t( m->bytes ), hipMemcpyHostToDevice ) );
		p.sq_serial = sq->img.serial;
	}
	const uint8_t	*tab = nullptr;
	int	codes = 0;
	if( letters_on_device( s, db, letters, &tab, &codes, err, errlen ) ||
		check_records( s, db, sc->prog, d_hits, n_hits, stream, false, nullptr, 0, err, errlen ) )
		return 1;
	char	*base = p.d_sq.as<char>();
	unsigned long long	*d_words = reinterpret_cast<unsigned long long *>( base ), *h_words = p.h_sq.as<unsigned long long>();
	RmqResult	*d_detail = reinterpret_cast<RmqResult *>( base + SQ_DETAIL_AT );
	RmqResult	*h_detail = reinterpret_cast<RmqResult *>( p.h_sq.as<char>() + SQ_DETAIL_AT );
	uint8_t	*keep = reinterpret_cast<uint8_t *>( base + SQ_RESULTS_AT );
	int32_t	*fixed = d_fixed != nullptr ? reinterpret_cast<int32_t *>( base + SQ_RESULTS_AT + flags ) : nullptr;
	HIPCHK( hipMemsetAsync( d_words, 0xff, 2 * sizeof( unsigned long long ), st ) );
	auto batch = [&]( int64_t c0, int64_t cn, RmqResult *detail ){
		return rma::SeqBatch{ p.d_sq_image.as<void>(), m->bytes, m->frames, d_hits + c0 * stride, ( long long )cn, ( long long )c0, stride,
			rma::hitwin_shape( sc->prog ), db->d_slen, db->d_text_start, db->n_seq, db->text, tab, codes, budget,
			keep + c0, detail == nullptr && fixed != nullptr ? fixed + c0 * stride : nullptr, d_words, d_words + 1, detail };
	};
	for( int64_t c0 = 0; c0 < n_hits; c0 += HW_CHUNK )
		HIPCHK( rma::seqcheck_records( batch( c0, std::min( HW_CHUNK, n_hits - c0 ), nullptr ), st ) );
	HIPCHK( hipMemcpyAsync( h_words, d_words, 2 * sizeof( unsigned long long ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipStreamSynchronize( st ) );
	if( h_words[ 0 ] != ~0ull )
		return bad_record( s, db, sc->prog, d_hits, int64_t( h_words[ 0 ] ), nullptr, "written", err, errlen );
	if( h_words[ 1 ] != ~0ull ){
		const int64_t	h = int64_t( h_words[ 1 ] );
		memset( h_detail, 0, sizeof( RmqResult ) );
		HIPCHK( hipMemsetAsync( d_detail, 0, sizeof( RmqResult ), st ) );
		HIPCHK( rma::seqcheck_records( batch( h, 1, d_detail ), st ) );
		HIPCHK( hipMemcpyAsync( h_detail, d_detail, sizeof( RmqResult ), hipMemcpyDeviceToHost, st ) );
		HIPCHK( hipStreamSynchronize( st ) );
		snprintf( err, errlen, "%s: record %lld: element %d: its seq= takes more than the budget of %d steps: nothing written", who, ( long long )h,
			h_detail->elem, budget );
		return 1;
	}
	HIPCHK( hipMemcpyAsync( d_keep, keep, n, hipMemcpyDeviceToDevice, st ) );
	if( d_fixed != nullptr )
		HIPCHK( hipMemcpyAsync( d_fixed, fixed, size_t( row_bytes ), hipMemcpyDeviceToDevice, st ) );
	return rma::stream_after( caller, st, err, errlen );
}

extern "C" void rma_seqcheck_info( const rma_seqcheck_t *sq, int32_t info[ 8 ] )
{
	if( sq == nullptr ){
		for( int i = 0; i < 8; i++ )
			info[ i ] = -1;
		return;
	}
	const RmqImage	*m = sq->img.image();
	const int	waves = rma::seqcheck_waves( m->bytes, m->frames );
	info[ 0 ] = m->n_expr;
	info[ 1 ] = m->n_ops;
	info[ 2 ] = m->frames;
	info[ 3 ] = m->bytes;
	info[ 4 ] = waves;
	info[ 5 ] = m->bytes + RMQ_LDS_TABLES + waves * rmq_wave_bytes( m->frames );
	int	priv = -1, lds = -1, regs = -1;
	if( rma::seqcheck_kernel_attributes( &priv, &lds, &regs ) != hipSuccess )
		( void )hipGetLastError();
	info[ 6 ] = priv;
	info[ 7 ] = regs;
}

// ---------------------------------------------------------------- the names of a database's entries on the device
// rma_names_create(): every sid and sdef of a database as one run of bytes and 2 n + 1 offsets (rm_hitprint_dev.h), copied
// once, on the upload stream of the database's device behind the database's own words.  The host copies stay with the
// table: the copies read them.  rma_names_destroy() waits for the upload and for the last kernel that read the table.
struct rma_names {
	const rma_db	*db = nullptr;	// (for the words of a refusal only: the database may be gone)
	uint64_t	db_serial = 0;	// rma_db::serial of the database the table was made for
	int	device = 0;
	int32_t	n = 0;
	std::vector<int64_t>	h_off;
	std::vector<uint8_t>	h_bytes;
	rma::DevMem	d_off, d_bytes;
	rma::Event	ready;		// the upload is complete (recorded on the upload stream)
	rma::Event	used;		// behind the last kernels that read the table
};

extern "C" void rma_names_destroy( rma_names_t *names )
{
	if( names == nullptr )
		return;
	( void )hipSetDevice( names->device );
	if( names->ready.get() != nullptr )
		( void )hipEventSynchronize( names->ready.get() );
	if( names->used.get() != nullptr )
		( void )hipEventSynchronize( names->used.get() );
	delete names;
}

extern "C" int rma_names_create( rma_scanner_t *sc, const rma_db_t *db, const char *const *sids, const int64_t *sid_len,
	const char *const *sdefs, const int64_t *sdef_len, int32_t n, rma_names_t **out, char *err, size_t errlen )
{
	const char	*who = "rma_names_create";
	if( out != nullptr )
		*out = nullptr;
	if( sc == nullptr || db == nullptr || out == nullptr ){
		snprintf( err, errlen, "%s: no %s", who, sc == nullptr ? "scanner" : db == nullptr ? "database" : "room for the table" );
		return 1;
	}
	if( !rma::is_device_db( db ) ){
		snprintf( err, errlen, "%s: the database (%p) was not made by rma_db_create_device() or has been destroyed", who,
			static_cast<const void *>( db ) );
		return 1;
	}
	if( db->device != sc->device ){
		snprintf( err, errlen, "%s: the database is on device %d, the scanner on device %d", who, db->device, sc->device );
		return 1;
	}
	if( n != db->n_seq ){
		snprintf( err, errlen, "%s: names of %d entries, the database has %d", who, n, db->n_seq );
		return 1;
	}
	std::unique_ptr<rma_names, void ( * )( rma_names * )>	made( new rma_names, rma_names_destroy );
	rma_names	*t = made.get();
	t->db = db;
	t->db_serial = db->serial;
	t->device = db->device;
	t->n = n;
	t->h_off.reserve( 2 * size_t( n ) + 1 );
	t->h_off.push_back( 0 );
	// one name: the caller's (a length given: no NUL inside it), or the default
	auto add = [&]( const char *p, const int64_t *len, int e, const std::string &dflt, const char *what ) -> int {
		int64_t	m = int64_t( dflt.size() );
		if( p == nullptr )
			p = dflt.data();
		else if( len == nullptr )
			m = int64_t( strlen( p ) );
		else{
			m = len[ e ];
			const void	*nul = m > 0 ? memchr( p, 0, size_t( m ) ) : nullptr;
			if( m < 0 || nul != nullptr ){
				if( m < 0 )
					snprintf( err, errlen, "%s: entry %d: its %s has a length of %lld", who, e, what, ( long long )m );
				else
					snprintf( err, errlen, "%s: entry %d: its %s has a NUL at byte %lld of %lld: rnamotif would print it up to there", who, e, what,
						( long long )( static_cast<const char *>( nul ) - p ), ( long long )m );
				return 1;
			}
		}
		t->h_bytes.insert( t->h_bytes.end(), p, p + m );
		t->h_off.push_back( int64_t( t->h_bytes.size() ) );
		return 0;
	};
	const bool	own = db->sids.size() == size_t( n ) && db->sdefs.size() == size_t( n );
	for( int e = 0; e < n; e++ ){
		// the defaults are the replay's: the entry's number, no definition -- or the names the database has read itself
		// (for one missing name among given ones as for a missing array)
		const std::string	sid = own ? db->sids[ size_t( e ) ] : std::to_string( e );
		const std::string	sdef = own ? db->sdefs[ size_t( e ) ] : std::string();
		if( add( sids != nullptr ? sids[ e ] : nullptr, sid_len, e, sid, "name" ) )
			return 1;
		const int64_t	m = t->h_off.back() - t->h_off[ t->h_off.size() - 2 ];
		if( m > rma::HP_MAX_SID ){
			snprintf( err, errlen, "%s: entry %d: its name has %lld bytes: rnamotif prints the first %d of a name, which the device does not restate",
				who, e, ( long long )m, rma::HP_MAX_SID );
			return 1;
		}
		if( add( sdefs != nullptr ? sdefs[ e ] : nullptr, sdef_len, e, sdef, "definition" ) )
			return 1;
	}
	HIPCHK( hipSetDevice( db->device ) );
	HIPCHK( t->d_off.exact( t->h_off.size() * sizeof( int64_t ) ) );
	HIPCHK( t->d_bytes.exact( std::max<size_t>( t->h_bytes.size(), 256 ) ) );
	HIPCHK( t->ready.create( hipEventDisableTiming ) );
	HIPCHK( t->used.create( hipEventDisableTiming ) );
	hipStream_t	up = rma::upload_stream( db );
	HIPCHK( hipStreamWaitEvent( up, db->ready.get(), 0 ) );
	HIPCHK( hipMemcpyAsync( t->d_off.as<void>(), t->h_off.data(), t->h_off.size() * sizeof( int64_t ), hipMemcpyHostToDevice, up ) );
	if( !t->h_bytes.empty() )
		HIPCHK( hipMemcpyAsync( t->d_bytes.as<void>(), t->h_bytes.data(), t->h_bytes.size(), hipMemcpyHostToDevice, up ) );
	HIPCHK( hipEventRecord( t->ready.get(), up ) );
	*out = made.release();
	return 0;
}

// ---------------------------------------------------------------- hit records as rnamotif prints them
// rma_hit_print_size() / rma_hit_print(): the size kernel of rm_hitprint_dev.hip and the scan of rm_hitwin_dev.hip in
// chunks of HW_CHUNK records, then the fill kernel, on the stream of the scanner's span scratch as rma_hit_structures
// runs its kernels: a chunk's offsets count from its first record, the bytes of the chunks before it wait in a word on
// the device (*hs_carry), so no chunk needs the host.  The size kernel checks each record, so the calls have no pass of
// their own for the check.  Words of the scratch's d_bad (rm_hitpost.h): HB_RECORD the least index of a bad record,
// HB_PRINT_TEXT of a bad text_len; HB_PRINT_SPARE, HB_PRINT_TEXT_SPARE where the fill call's second pass over a later
// chunk puts them (the same records, already judged).
namespace {

struct PrintCall {
	rma_scanner_t	*sc;
	const rma_db	*db;
	rma_names	*names;
	const int32_t	*d_hits;
	int64_t	n_hits;
	const uint8_t	*d_accept;
	const int32_t	*d_text_len;
	int32_t	text_width;
};

rma::HitPrintBatch print_batch( const PrintCall &c, int64_t c0, int64_t cn )
{
	const int	stride = rma_hit_stride( &c.sc->prog );
	return rma::HitPrintBatch{ c.d_hits + c0 * stride, ( long long )cn, ( long long )c0, stride, rma::hitwin_shape( c.sc->prog ), c.db->d_slen,
		c.db->d_text_start, c.db->n_seq, c.d_accept != nullptr ? c.d_accept + c0 : nullptr, c.d_text_len + c0, c.text_width,
		rma::HitPrintNames{ c.names->d_bytes.as<uint8_t>(), c.names->d_off.as<int64_t>() } };
}

// What both calls do first: the scanner, the database, the records, the names and the two inputs every record has.
int hit_print_args( const char *who, const PrintCall &c, char *err, size_t errlen )
{
	if( c.sc == nullptr || c.db == nullptr || c.names == nullptr ){
		snprintf( err, errlen, "%s: no %s", who, c.sc == nullptr ? "scanner" : c.db == nullptr ? "database" : "names" );
		return 1;
	}
	if( hit_structures_args( c.sc, c.db, c.d_hits, c.n_hits, who, err, errlen ) )
		return 1;
	// (by the database's serial number: a later database may lie where the table's lay)
	if( c.names->db_serial != c.db->serial || c.names->n != c.db->n_seq ){
		snprintf( err, errlen, "%s: the names were made for another database (%p) than this one (%p): nothing printed", who,
			static_cast<const void *>( c.names->db ), static_cast<const void *>( c.db ) );
		return 1;
	}
	if( c.n_hits == 0 )
		return 0;
	if( c.d_text_len == nullptr ){
		snprintf( err, errlen, "%s: %lld records: bad arguments", who, ( long long )c.n_hits );
		return 1;
	}
	if( rma::check_device_bytes( c.d_text_len, c.sc->device, 0, c.n_hits * 4, "the text's lengths", err, errlen ) ||
		( c.d_accept != nullptr && rma::check_device_bytes( c.d_accept, c.sc->device, 0, c.n_hits, "the accept flags", err, errlen ) ) )
		return 1;
	return 0;
}

// One chunk's sizes and offsets into the scratch; the bad words as hit_print_sizes takes them
int hit_print_sizes_of( const PrintCall &c, int64_t c0, int64_t cn, unsigned long long *bad, unsigned long long *bad_text, char *err, size_t errlen )
{
	rma::HitWindowScratch	*s = c.sc->post->win;
	HIPCHK( rma::hit_print_sizes( print_batch( c, c0, cn ), s->d_len, bad, bad_text, s->stream.get() ) );
	size_t	tb = s->d_tmp.bytes();
	HIPCHK( rma::hit_offsets( s->d_len, s->d_off, cn + 1, s->d_tmp.as<void>(), &tb, s->stream.get() ) );
	return 0;
}

// Every record checked on the device and the bytes of their lines counted (n_hits > 0, hit_print_args has passed): one
// synchronisation.  A call of one chunk leaves that chunk's offsets in the scratch.
int hit_print_count( const char *who, const PrintCall &c, void *stream, int64_t *total, char *err, size_t errlen )
{
	rma::HitPost	&p = *c.sc->post;
	rma::HitWindowScratch	*s = p.win;
	hipStream_t	st = s->stream.get();
	if( check_records( s, c.db, c.sc->prog, c.d_hits, c.n_hits, stream, false, p.hs_carry(), sizeof( int64_t ), err, errlen ) )
		return 1;
	HIPCHK( hipStreamWaitEvent( st, c.names->ready.get(), 0 ) );
	HIPCHK( hipMemsetAsync( s->d_bad + rma::HB_PRINT_TEXT, 0xff, sizeof( unsigned long long ), st ) );
	for( int64_t c0 = 0; c0 < c.n_hits; c0 += HW_CHUNK ){
		const int64_t	cn = std::min( HW_CHUNK, c.n_hits - c0 );
		if( hit_print_sizes_of( c, c0, cn, s->d_bad + rma::HB_RECORD, s->d_bad + rma::HB_PRINT_TEXT, err, errlen ) )
			return 1;
		HIPCHK( rma::hit_carry_add( p.hs_carry(), s->d_off + cn, st ) );
	}
	HIPCHK( hipMemcpyAsync( s->h_bad + rma::HBH_FIRST, s->d_bad + rma::HB_RECORD, sizeof( unsigned long long ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipMemcpyAsync( s->h_bad + rma::HBH_TOTAL, p.hs_carry(), sizeof( int64_t ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipMemcpyAsync( s->h_bad + rma::HBH_SECOND, s->d_bad + rma::HB_PRINT_TEXT, sizeof( unsigned long long ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipEventRecord( c.names->used.get(), st ) );
	HIPCHK( hipStreamSynchronize( st ) );
	if( s->h_bad[ rma::HBH_FIRST ] != ~0ull )
		return bad_record( s, c.db, c.sc->prog, c.d_hits, int64_t( s->h_bad[ rma::HBH_FIRST ] ), nullptr, "printed", err, errlen );
	if( s->h_bad[ rma::HBH_SECOND ] != ~0ull ){
		const int64_t	h = int64_t( s->h_bad[ rma::HBH_SECOND ] );
		int32_t	len = 0;
		HIPCHK( hipMemcpyAsync( &len, c.d_text_len + h, sizeof( len ), hipMemcpyDeviceToHost, st ) );
		HIPCHK( hipStreamSynchronize( st ) );
		if( c.text_width == INT32_MAX )
			snprintf( err, errlen, "%s: record %lld: a score column of %d bytes: nothing printed", who, ( long long )h, len );
		else
			snprintf( err, errlen, "%s: record %lld: a score column of %d bytes, outside the [0, %d] of text_width: nothing printed", who,
				( long long )h, len, c.text_width );
		return 1;
	}
	*total = int64_t( s->h_bad[ rma::HBH_TOTAL ] );
	return 0;
}

}	// namespace

extern "C" int rma_hit_print_size( rma_scanner_t *sc, const rma_db_t *db, const rma_names_t *names, const int32_t *d_hits, int64_t n_hits,
	const uint8_t *d_accept, const int32_t *d_text_len, int64_t *total, void *stream, char *err, size_t errlen )
{
	const char	*who = "rma_hit_print_size";
	if( total == nullptr ){
		snprintf( err, errlen, "%s: no room for the total", who );
		return 1;
	}
	*total = 0;
	// (the size call knows no row width: any length from 0 passes here, the fill call holds it to its text_width)
	const PrintCall	c{ sc, db, const_cast<rma_names_t *>( names ), d_hits, n_hits, d_accept, d_text_len, INT32_MAX };
	if( hit_print_args( who, c, err, errlen ) )
		return 1;
	return n_hits == 0 ? 0 : hit_print_count( who, c, stream, total, err, errlen );
}

extern "C" int rma_hit_print( rma_scanner_t *sc, const rma_db_t *db, const rma_names_t *names, const int32_t *d_hits, int64_t n_hits,
	const uint8_t *letters, const uint8_t *d_accept, const uint8_t *d_text_bytes, int32_t text_width, const int32_t *d_text_len,
	int64_t total, uint8_t *d_out, int64_t *d_off, void *stream, char *err, size_t errlen )
{
	const char	*who = "rma_hit_print";
	const PrintCall	c{ sc, db, const_cast<rma_names_t *>( names ), d_hits, n_hits, d_accept, d_text_len, text_width };
	if( hit_print_args( who, c, err, errlen ) )
		return 1;
	if( total < 0 || total > INT64_MAX / 16 || d_off == nullptr || ( total > 0 && d_out == nullptr ) || text_width < 0 ||
		( n_hits > 0 && text_width > 0 && ( d_text_bytes == nullptr || n_hits > ( int64_t( 1 ) << 40 ) / text_width ) ) ){
		snprintf( err, errlen, "%s: %lld bytes, score columns in rows of %d bytes: bad arguments", who, ( long long )total, text_width );
		return 1;
	}
	// the outputs and the score columns: the caller's, each inside its allocation on the scanner's device
	if( rma::check_device_bytes( d_off, sc->device, 0, ( n_hits + 1 ) * 8, "the offsets", err, errlen ) ||
		( total > 0 && rma::check_device_bytes( d_out, sc->device, 0, total, "the printed bytes", err, errlen ) ) ||
		( n_hits > 0 && text_width > 0 && rma::check_device_bytes( d_text_bytes, sc->device, 0, n_hits * text_width, "the score columns", err, errlen ) ) )
		return 1;
	hipStream_t	caller = static_cast<hipStream_t>( stream );
	int64_t	found = 0;
	const uint8_t	*tab = nullptr;
	int	codes = 0;
	// the letters as rma_hit_structures takes them, on their way ahead of the count, whose synchronisation leaves the
	// page-locked copy free for the next call
	if( n_hits > 0 && ( letters_on_device( sc->post->win, db, letters, &tab, &codes, err, errlen ) ||
		hit_print_count( who, c, stream, &found, err, errlen ) ) )
		return 1;
	if( found != total ){
		snprintf( err, errlen, "%s: the lines of the %lld records have %lld bytes, not the %lld of `total`: nothing printed", who,
			( long long )n_hits, ( long long )found, ( long long )total );
		return 1;
	}
	if( n_hits == 0 ){
		HIPCHK( hipMemsetAsync( d_off, 0, sizeof( int64_t ), caller ) );
		return 0;
	}
	rma::HitPost	&p = *sc->post;
	rma::HitWindowScratch	*s = p.win;
	hipStream_t	st = s->stream.get();
	HIPCHK( hipMemsetAsync( p.hs_carry(), 0, sizeof( int64_t ), st ) );
	for( int64_t c0 = 0; c0 < n_hits; c0 += HW_CHUNK ){
		const int64_t	cn = std::min( HW_CHUNK, n_hits - c0 );
		// (a call of one chunk: the count's offsets are still there)
		if( n_hits > HW_CHUNK && hit_print_sizes_of( c, c0, cn, s->d_bad + rma::HB_PRINT_SPARE, s->d_bad + rma::HB_PRINT_TEXT_SPARE, err, errlen ) )
			return 1;
		HIPCHK( rma::hit_print_fill( print_batch( c, c0, cn ), db->text, tab, codes, d_text_bytes, s->d_off, p.hs_carry(), d_out, d_off + c0,
			c0 + cn == n_hits, st ) );
		HIPCHK( rma::hit_carry_add( p.hs_carry(), s->d_off + cn, st ) );
	}
	HIPCHK( hipEventRecord( names->used.get(), st ) );
	return rma::stream_after( caller, st, err, errlen );
}

// ---------------------------------------------------------------- hit records as rmfmt lists them
// rma_hit_list_shape() / rma_hit_list(): the kernels of rm_hitlist_dev.hip on the stream of the scanner's span scratch,
// as rma_hit_print runs its own.  Both calls measure: every record checked and measured in chunks of HW_CHUNK, a chunk's
// flags scanned (hit_offsets) and its printed records' indices compacted behind those of the chunks before it (the
// running count waits in *hs_carry), the call's sums reduced into one block; one wait brings the sums back, and with
// them the listing's mode, lines and widths or the least refused record.  rma_hit_list then queues the sort of the
// indices into the caller's permutation and the fill, and returns.  The scratch is the scanner's: one fixed block (the
// sums, the layout, the letters with their complements) on the device and one page-locked (the sums to start from,
// the sums found, the layout), and per call the measured records, the indices and the sort's work area, grown behind a
// wait for the kernels that read them.
namespace {

constexpr size_t	HL_AT_RESULT = 1024, HL_AT_LAYOUT = 2048, HL_AT_LETTERS = 3072, HL_FIXED_BYTES = 4096;
static_assert( sizeof( rma::HitListSums ) <= HL_AT_RESULT && sizeof( rma::HitListLayout ) <= HL_AT_LETTERS - HL_AT_LAYOUT, "the fixed block's slots" );

struct ListCall {
	rma_scanner_t	*sc;
	const rma_db	*db;
	rma_names	*names;
	const int32_t	*d_hits;
	int64_t	n_hits;
	const uint8_t	*d_accept, *d_text_bytes;
	int32_t	text_width;
	const int32_t	*d_text_len;
	int	name_mode;
	int64_t	smax;
};

struct ListShape {
	int64_t	n_lines;
	int	mode, k;
	int32_t	widths[ rma::HL_MAX_SEGS ];
	rma::HitListLayout	layout;
};

// a scratch piece with room for `want` bytes: grown only behind the kernels that read what is there
int list_room( rma::DevMem &m, size_t want, hipStream_t st, char *err, size_t errlen )
{
	if( want <= m.bytes() )
		return 0;
	HIPCHK( hipStreamSynchronize( st ) );
	HIPCHK( m.room( want ) );
	return 0;
}

// The first entry whose name is no field of its hit line for a tool that splits the line at blanks: one that is empty,
// trims to nothing (name_mode) or holds a blank, a tab or a newline -- any_space: or another of isspace()'s bytes; -1: none.
int32_t names_first_split( const rma_names &names, int name_mode, bool any_space )
{
	for( int32_t e = 0; e < names.n; e++ ){
		const int64_t	lo = names.h_off[ 2 * size_t( e ) ], m = names.h_off[ 2 * size_t( e ) + 1 ] - lo;
		const uint8_t	*sid = names.h_bytes.data() + lo;
		int32_t	at;
		bool	bad = rma::rmlist_name( sid, int32_t( m ), name_mode, &at ) == 0;
		for( int64_t j = 0; j < m && !bad; j++ )
			bad = sid[ j ] == ' ' || sid[ j ] == '\t' || sid[ j ] == '\n' || ( any_space && ( sid[ j ] == '\v' || sid[ j ] == '\f' || sid[ j ] == '\r' ) );
		if( bad )
			return e;
	}
	return -1;
}

// What both calls do first: the scanner, the database, the records, the names, the inputs every record has -- and what
// the host knows of the names: rmfmt splits a line at every blank, so a name with one in it, or one that is or trims to
// nothing, is no field of its line.
int hit_list_args( const char *who, const ListCall &c, char *err, size_t errlen )
{
	if( c.sc == nullptr || c.db == nullptr || c.names == nullptr ){
		snprintf( err, errlen, "%s: no %s", who, c.sc == nullptr ? "scanner" : c.db == nullptr ? "database" : "names" );
		return 1;
	}
	if( hit_structures_args( c.sc, c.db, c.d_hits, c.n_hits, who, err, errlen ) )
		return 1;
	if( c.names->db_serial != c.db->serial || c.names->n != c.db->n_seq ){
		snprintf( err, errlen, "%s: the names were made for another database (%p) than this one (%p): nothing printed", who,
			static_cast<const void *>( c.names->db ), static_cast<const void *>( c.db ) );
		return 1;
	}
	if( c.name_mode != rma::HL_WHOLE && c.name_mode != rma::HL_LOCUS && c.name_mode != rma::HL_ACC ){
		snprintf( err, errlen, "%s: name mode %d: RMA_LIST_WHOLE, RMA_LIST_LOCUS or RMA_LIST_ACC", who, c.name_mode );
		return 1;
	}
	if( c.n_hits == 0 )
		return 0;
	if( c.d_text_len == nullptr || c.text_width < 0 || ( c.text_width > 0 && ( c.d_text_bytes == nullptr || c.n_hits > ( int64_t( 1 ) << 40 ) / c.text_width ) ) ){
		snprintf( err, errlen, "%s: %lld records, score columns in rows of %d bytes: bad arguments", who, ( long long )c.n_hits, c.text_width );
		return 1;
	}
	if( rma::check_device_bytes( c.d_text_len, c.sc->device, 0, c.n_hits * 4, "the text's lengths", err, errlen ) ||
		( c.d_accept != nullptr && rma::check_device_bytes( c.d_accept, c.sc->device, 0, c.n_hits, "the accept flags", err, errlen ) ) ||
		( c.text_width > 0 && rma::check_device_bytes( c.d_text_bytes, c.sc->device, 0, c.n_hits * c.text_width, "the score columns", err, errlen ) ) )
		return 1;
	const int32_t	e = names_first_split( *c.names, c.name_mode, false );
	if( e >= 0 ){
		snprintf( err, errlen, "%s: entry %d: its name is empty, trims to nothing or has a blank, a tab or a newline in it: rmfmt would split the line there: nothing listed",
			who, e );
		return 1;
	}
	return 0;
}

rma::HitListCall list_call( const ListCall &c )
{
	rma::HitPost	&p = *c.sc->post;
	return rma::HitListCall{ c.d_hits, ( long long )c.n_hits, rma_hit_stride( &c.sc->prog ), rma::hitwin_shape( c.sc->prog ), c.db->d_slen,
		c.db->d_text_start, c.db->n_seq, c.d_accept, c.d_text_len, c.d_text_bytes, c.text_width,
		rma::HitPrintNames{ c.names->d_bytes.as<uint8_t>(), c.names->d_off.as<int64_t>() }, c.name_mode, p.d_hl_rec.as<rma::HitListRec>() };
}

// the first two printed records whose numbers of score fields differ (the measured records come to the host: a refusal's path)
int list_mixed( const char *who, const ListCall &c, hipStream_t st, char *err, size_t errlen )
{
	std::vector<rma::HitListRec>	recs( static_cast<size_t>( c.n_hits ) );
	HIPCHK( hipMemcpyAsync( recs.data(), c.sc->post->d_hl_rec.as<void>(), recs.size() * sizeof( rma::HitListRec ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipStreamSynchronize( st ) );
	int64_t	first = -1;
	for( int64_t h = 0; h < c.n_hits; h++ ){
		if( recs[ size_t( h ) ].k < 0 )
			continue;
		if( first < 0 )
			first = h;
		else if( recs[ size_t( h ) ].k != recs[ size_t( first ) ].k ){
			rma::rmlist_refusal_mixed( err, errlen, who, ( long long )first, recs[ size_t( first ) ].k, ( long long )h, recs[ size_t( h ) ].k );
			return 1;
		}
	}
	snprintf( err, errlen, "%s: refused on the device, not on the host (records changed during the call?)", who );
	return 1;
}

// Every record checked and measured on the device, the printed ones' indices compacted (n_hits > 0, hit_list_args has
// passed): one synchronisation.  *shape: what the listing is, or the words of the refusal.
int hit_list_measure_all( const char *who, const ListCall &c, void *stream, ListShape *shape, char *err, size_t errlen )
{
	rma::HitPost	&p = *c.sc->post;
	rma::HitWindowScratch	*s = p.win;
	hipStream_t	st = s->stream.get();
	if( !p.d_hl ){
		rma::DevMem	dev;
		rma::PinMem	pin;
		HIPCHK( dev.exact( HL_FIXED_BYTES ) );
		HIPCHK( pin.exact( HL_FIXED_BYTES ) );
		*pin.as<rma::HitListSums>() = rma::HitListSums::init();
		p.d_hl = std::move( dev );
		p.h_hl = std::move( pin );
	}
	if( list_room( p.d_hl_rec, size_t( c.n_hits ) * sizeof( rma::HitListRec ), st, err, errlen ) ||
		list_room( p.d_hl_idx, size_t( c.n_hits ) * sizeof( int64_t ), st, err, errlen ) )
		return 1;
	if( check_records( s, c.db, c.sc->prog, c.d_hits, c.n_hits, stream, false, p.hs_carry(), sizeof( int64_t ), err, errlen ) )
		return 1;
	HIPCHK( hipStreamWaitEvent( st, c.names->ready.get(), 0 ) );
	rma::HitListSums	*d_sums = p.d_hl.as<rma::HitListSums>();
	const rma::HitListSums	*found = reinterpret_cast<const rma::HitListSums *>( p.h_hl.as<char>() + HL_AT_RESULT );
	HIPCHK( hipMemcpyAsync( d_sums, p.h_hl.as<void>(), sizeof( rma::HitListSums ), hipMemcpyHostToDevice, st ) );
	const rma::HitListCall	call = list_call( c );
	for( int64_t c0 = 0; c0 < c.n_hits; c0 += HW_CHUNK ){
		const int64_t	cn = std::min( HW_CHUNK, c.n_hits - c0 );
		HIPCHK( rma::hit_list_measure( call, c0, cn, s->d_len, d_sums, st ) );
		size_t	tb = s->d_tmp.bytes();
		HIPCHK( rma::hit_offsets( s->d_len, s->d_off, cn + 1, s->d_tmp.as<void>(), &tb, st ) );
		HIPCHK( rma::hit_list_compact( s->d_len, s->d_off, p.hs_carry(), c0, cn, p.d_hl_idx.as<int64_t>(), st ) );
		HIPCHK( rma::hit_carry_add( p.hs_carry(), s->d_off + cn, st ) );
	}
	HIPCHK( hipMemcpyAsync( const_cast<rma::HitListSums *>( found ), d_sums, sizeof( rma::HitListSums ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipEventRecord( c.names->used.get(), st ) );
	HIPCHK( hipStreamSynchronize( st ) );
	if( found->bad != ~0ull ){
		const int64_t	h = int64_t( found->bad >> 4 );
		const int	code = int( found->bad & 15 );
		if( code < rma::HP_TEXT )
			return bad_record( s, c.db, c.sc->prog, c.d_hits, h, nullptr, "listed", err, errlen );
		if( code == rma::HP_TEXT ){
			int32_t	len = 0;
			HIPCHK( hipMemcpyAsync( &len, c.d_text_len + h, sizeof( len ), hipMemcpyDeviceToHost, st ) );
			HIPCHK( hipStreamSynchronize( st ) );
			snprintf( err, errlen, "%s: record %lld: a score column of %d bytes, outside the [0, %d] of text_width: nothing listed", who,
				( long long )h, len, c.text_width );
			return 1;
		}
		rma::rmlist_refusal( err, errlen, who, code, ( long long )h );
		return 1;
	}
	if( found->n_lines > 0 && found->k_min != found->k_max )
		return list_mixed( who, c, st, err, errlen );
	shape->n_lines = int64_t( found->n_lines );
	shape->k = shape->n_lines > 0 ? int( found->k_min ) : 1;
	shape->mode = int64_t( found->temp_bytes ) > c.smax ? 0 : shape->k == 1 && !found->not_number ? 1 : 2;
	for( int g = 0; g < rma::HL_MAX_SEGS; g++ )
		shape->widths[ g ] = int32_t( found->width[ g ] );
	return 0;
}

// the listing of no records
void list_nothing( ListShape *shape )
{
	shape->n_lines = 0;
	shape->mode = 1;
	shape->k = 1;
	memset( shape->widths, 0, sizeof( shape->widths ) );
}

// the layout of a measured listing; refused where a line would not fit the 32 bits of its offsets
int list_layout( const char *who, const rma_program_t &prog, ListShape *shape, char *err, size_t errlen )
{
	int64_t	sum = 0;
	for( int g = 0; g < rma::HL_MAX_SEGS; g++ )
		sum += int64_t( shape->widths[ g ] ) + 1;
	if( sum > INT32_MAX / 2 ){
		snprintf( err, errlen, "%s: lines of %lld bytes: nothing listed", who, ( long long )sum );
		return 1;
	}
	uint8_t	right[ rma::HA_MAX_COLS ];
	rma::hitalign_directions( prog, right );
	shape->layout = rma::rmlist_layout( rma::hitwin_shape( prog ), right, shape->widths, shape->k );
	return 0;
}

}	// namespace

extern "C" int rma_hit_list_shape( rma_scanner_t *sc, const rma_db_t *db, const rma_names_t *names, const int32_t *d_hits, int64_t n_hits,
	const uint8_t *d_accept, const uint8_t *d_text_bytes, int32_t text_width, const int32_t *d_text_len, int32_t name_mode, int64_t smax,
	int64_t *n_lines, int64_t *line_len, int32_t *widths, int32_t *mode, void *stream, char *err, size_t errlen )
{
	const char	*who = "rma_hit_list_shape";
	if( n_lines == nullptr || line_len == nullptr || widths == nullptr || mode == nullptr ){
		snprintf( err, errlen, "%s: no room for the shape", who );
		return 1;
	}
	const ListCall	c{ sc, db, const_cast<rma_names_t *>( names ), d_hits, n_hits, d_accept, d_text_bytes, text_width, d_text_len, name_mode,
		smax > 0 ? smax : rma::HL_SMAX };
	if( hit_list_args( who, c, err, errlen ) )
		return 1;
	ListShape	shape;
	list_nothing( &shape );
	if( n_hits > 0 && hit_list_measure_all( who, c, stream, &shape, err, errlen ) )
		return 1;
	if( list_layout( who, sc->prog, &shape, err, errlen ) )
		return 1;
	*n_lines = shape.n_lines;
	*line_len = shape.layout.line_len;
	*mode = shape.mode;
	memcpy( widths, shape.widths, sizeof( shape.widths ) );
	return 0;
}

extern "C" int rma_hit_list( rma_scanner_t *sc, const rma_db_t *db, const rma_names_t *names, const int32_t *d_hits, int64_t n_hits,
	const uint8_t *d_accept, const uint8_t *d_text_bytes, int32_t text_width, const int32_t *d_text_len, int32_t name_mode, int64_t smax,
	const uint8_t *letters, int64_t n_lines, int64_t line_len, uint8_t *d_lines, int64_t *d_perm, void *stream, char *err, size_t errlen )
{
	const char	*who = "rma_hit_list";
	const ListCall	c{ sc, db, const_cast<rma_names_t *>( names ), d_hits, n_hits, d_accept, d_text_bytes, text_width, d_text_len, name_mode,
		smax > 0 ? smax : rma::HL_SMAX };
	if( hit_list_args( who, c, err, errlen ) )
		return 1;
	if( letters != nullptr )
		for( int b = 0; b < 256; b++ )
			if( letters[ b ] == ' ' || letters[ b ] == '\t' || letters[ b ] == '\n' ){
				snprintf( err, errlen, "%s: the letters map byte %d to a blank, a tab or a newline: nothing listed", who, b );
				return 1;
			}
	if( n_lines < 0 || line_len < 0 || n_lines > n_hits || ( n_lines > 0 && ( d_lines == nullptr || d_perm == nullptr || line_len > INT64_MAX / 16 / n_lines ) ) ){
		snprintf( err, errlen, "%s: %lld lines of %lld bytes: bad arguments", who, ( long long )n_lines, ( long long )line_len );
		return 1;
	}
	// the outputs: the caller's, each inside its allocation on the scanner's device
	if( n_lines > 0 && ( ( line_len > 0 && rma::check_device_bytes( d_lines, sc->device, 0, n_lines * line_len, "the lines", err, errlen ) ) ||
		rma::check_device_bytes( d_perm, sc->device, 0, n_lines * 8, "the permutation", err, errlen ) ) )
		return 1;
	ListShape	shape;
	list_nothing( &shape );
	const uint8_t	*tab = nullptr;
	int	codes = 0;
	// the letters as rma_hit_print takes them, on their way ahead of the measure pass, whose synchronisation leaves the
	// page-locked copy free for the next call
	if( n_hits > 0 && ( letters_on_device( sc->post->win, db, letters, &tab, &codes, err, errlen ) ||
		hit_list_measure_all( who, c, stream, &shape, err, errlen ) ) )
		return 1;
	if( list_layout( who, sc->prog, &shape, err, errlen ) )
		return 1;
	if( shape.n_lines != n_lines || shape.layout.line_len != line_len ){
		snprintf( err, errlen, "%s: the listing of the %lld records has %lld lines of %d bytes, not the %lld lines of %lld bytes given: nothing listed", who,
			( long long )n_hits, ( long long )shape.n_lines, shape.layout.line_len, ( long long )n_lines, ( long long )line_len );
		return 1;
	}
	if( n_lines == 0 )
		return 0;
	rma::HitPost	&p = *sc->post;
	hipStream_t	st = p.win->stream.get(), caller = static_cast<hipStream_t>( stream );
	const rma::HitListCall	call = list_call( c );
	const int64_t	*d_idx = p.d_hl_idx.as<int64_t>();
	uint8_t	*d_letcmp = p.d_hl.as<uint8_t>() + HL_AT_LETTERS;
	const rma::HitListLayout	*d_layout = reinterpret_cast<const rma::HitListLayout *>( p.d_hl.as<char>() + HL_AT_LAYOUT );
	// (the page-locked layout is free: the call before this one has had its copy made by the time the measure pass's wait ended)
	memcpy( p.h_hl.as<char>() + HL_AT_LAYOUT, &shape.layout, sizeof( shape.layout ) );
	HIPCHK( hipMemcpyAsync( const_cast<rma::HitListLayout *>( d_layout ), p.h_hl.as<char>() + HL_AT_LAYOUT, sizeof( shape.layout ), hipMemcpyHostToDevice, st ) );
	HIPCHK( rma::hit_list_letters( tab, codes, d_letcmp, st ) );
	if( shape.mode == 0 )
		HIPCHK( hipMemcpyAsync( d_perm, d_idx, size_t( n_lines ) * 8, hipMemcpyDeviceToDevice, st ) );
	else{
		// (the library picks its algorithm by size: what a small sort needs is not bounded by the largest one's)
		size_t	bytes = 0;
		HIPCHK( rma::hit_list_sort( call, db->text, d_letcmp, shape.mode, d_idx, d_perm, n_lines, nullptr, &bytes, st ) );
		if( list_room( p.d_hl_tmp, std::max<size_t>( bytes, 256 ), st, err, errlen ) )
			return 1;
		bytes = p.d_hl_tmp.bytes();
		HIPCHK( rma::hit_list_sort( call, db->text, d_letcmp, shape.mode, d_idx, d_perm, n_lines, p.d_hl_tmp.as<void>(), &bytes, st ) );
	}
	HIPCHK( rma::hit_list_fill( call, db->text, d_letcmp, d_layout, shape.layout.line_len, d_perm, n_lines, d_lines, st ) );
	HIPCHK( hipEventRecord( names->used.get(), st ) );
	return rma::stream_after( caller, st, err, errlen );
}

// ---------------------------------------------------------------- hit records as rm2ct writes them
// rma_hit_ct_size() / rma_hit_ct(): the size kernel of rm_hitct_dev.hip and the scan of rm_hitwin_dev.hip in chunks of
// HW_CHUNK records, then the fill kernel, on the stream of the scanner's span scratch with the running total in
// *hs_carry, as rma_hit_print runs its own.  The descriptor's table (rm_hitct.h) is made per call from the words of the
// "#RM descr" line and goes to the kernels with their arguments.  Words of the scratch's d_bad (rm_hitpost.h): HB_CT the
// least refused record with its reason, HB_CT_SPARE where the fill call's second pass over a later chunk puts it (the
// same records, already judged).
namespace {

struct CtCall {
	PrintCall	p;
	const uint8_t	*d_text_bytes;
	int32_t	type;
	rma::HitCtTable	table;
};

rma::HitCtBatch ct_batch( const CtCall &c, int64_t c0, int64_t cn )
{
	return rma::HitCtBatch{ print_batch( c.p, c0, cn ), c.d_text_bytes, c.type, c.table };
}

// What both calls do first: rma_hit_print's arguments, then what rm2ct refuses or would misread before it has seen a
// record -- a triple or quad helix, a type it does not know, a name it would cut, letters it would not count as bases.
int hit_ct_args( const char *who, CtCall *c, const char *descr_words, const uint8_t *letters, char *err, size_t errlen )
{
	const PrintCall	&p = c->p;
	if( hit_print_args( who, p, err, errlen ) )
		return 1;
	if( descr_words == nullptr ){
		snprintf( err, errlen, "%s: no words of the \"#RM descr\" line (rma_descr_names)", who );
		return 1;
	}
	char	why[ 256 ];
	if( rma::hitct_table( descr_words, rma::hitalign_n_cols( rma::hitwin_shape( p.sc->prog ) ), &c->table, why, sizeof( why ) ) ){
		snprintf( err, errlen, "%s: %s", who, why );
		return 1;
	}
	if( c->type != rma::HC_RNAMOTIF && c->type != rma::HC_RNAVIZ ){
		snprintf( err, errlen, "%s: type %d: RMA_CT_RNAMOTIF or RMA_CT_RNAVIZ", who, c->type );
		return 1;
	}
	const int32_t	e = names_first_split( *p.names, rma::HL_WHOLE, true );
	if( e >= 0 ){
		snprintf( err, errlen, "%s: entry %d: its name is empty or has a blank, a tab, a newline or another space in it: rm2ct would cut the name there: nothing written",
			who, e );
		return 1;
	}
	if( letters != nullptr )
		for( int b = 0; b < 256; b++ )
			if( !( ( letters[ b ] >= 'a' && letters[ b ] <= 'z' ) || ( letters[ b ] >= 'A' && letters[ b ] <= 'Z' ) ) ){
				snprintf( err, errlen, "%s: the letters map byte %d to %d, which is no ASCII letter: rm2ct counts bases with isalpha(): nothing written", who, b,
					int( letters[ b ] ) );
				return 1;
			}
	if( p.n_hits == 0 )
		return 0;
	if( p.text_width < 0 || ( p.text_width > 0 && ( c->d_text_bytes == nullptr || p.n_hits > ( int64_t( 1 ) << 40 ) / p.text_width ) ) ){
		snprintf( err, errlen, "%s: %lld records, score columns in rows of %d bytes: bad arguments", who, ( long long )p.n_hits, p.text_width );
		return 1;
	}
	if( p.text_width > 0 && rma::check_device_bytes( c->d_text_bytes, p.sc->device, 0, p.n_hits * p.text_width, "the score columns", err, errlen ) )
		return 1;
	return 0;
}

// One chunk's sizes and offsets into the scratch; the bad word as hit_ct_sizes takes it
int hit_ct_sizes_of( const CtCall &c, int64_t c0, int64_t cn, unsigned long long *bad, char *err, size_t errlen )
{
	rma::HitWindowScratch	*s = c.p.sc->post->win;
	HIPCHK( rma::hit_ct_sizes( ct_batch( c, c0, cn ), s->d_len, bad, s->stream.get() ) );
	size_t	tb = s->d_tmp.bytes();
	HIPCHK( rma::hit_offsets( s->d_len, s->d_off, cn + 1, s->d_tmp.as<void>(), &tb, s->stream.get() ) );
	return 0;
}

// Every record checked and measured on the device and the bytes of their .ct records counted (n_hits > 0, hit_ct_args has
// passed): one synchronisation.  A call of one chunk leaves that chunk's offsets in the scratch.
int hit_ct_count( const char *who, const CtCall &c, void *stream, int64_t *total, char *err, size_t errlen )
{
	const PrintCall	&pc = c.p;
	rma::HitPost	&p = *pc.sc->post;
	rma::HitWindowScratch	*s = p.win;
	hipStream_t	st = s->stream.get();
	if( check_records( s, pc.db, pc.sc->prog, pc.d_hits, pc.n_hits, stream, false, p.hs_carry(), sizeof( int64_t ), err, errlen ) )
		return 1;
	HIPCHK( hipStreamWaitEvent( st, pc.names->ready.get(), 0 ) );
	HIPCHK( hipMemsetAsync( s->d_bad + rma::HB_CT, 0xff, sizeof( unsigned long long ), st ) );
	for( int64_t c0 = 0; c0 < pc.n_hits; c0 += HW_CHUNK ){
		const int64_t	cn = std::min( HW_CHUNK, pc.n_hits - c0 );
		if( hit_ct_sizes_of( c, c0, cn, s->d_bad + rma::HB_CT, err, errlen ) )
			return 1;
		HIPCHK( rma::hit_carry_add( p.hs_carry(), s->d_off + cn, st ) );
	}
	HIPCHK( hipMemcpyAsync( s->h_bad + rma::HBH_FIRST, s->d_bad + rma::HB_CT, sizeof( unsigned long long ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipMemcpyAsync( s->h_bad + rma::HBH_TOTAL, p.hs_carry(), sizeof( int64_t ), hipMemcpyDeviceToHost, st ) );
	HIPCHK( hipEventRecord( pc.names->used.get(), st ) );
	HIPCHK( hipStreamSynchronize( st ) );
	if( s->h_bad[ rma::HBH_FIRST ] != ~0ull ){
		const int64_t	h = int64_t( s->h_bad[ rma::HBH_FIRST ] >> 4 );
		const int	code = int( s->h_bad[ rma::HBH_FIRST ] & 15 );
		if( code < rma::HP_TEXT )
			return bad_record( s, pc.db, pc.sc->prog, pc.d_hits, h, nullptr, "written", err, errlen );
		if( code == rma::HP_TEXT ){
			int32_t	len = 0;
			HIPCHK( hipMemcpyAsync( &len, pc.d_text_len + h, sizeof( len ), hipMemcpyDeviceToHost, st ) );
			HIPCHK( hipStreamSynchronize( st ) );
			snprintf( err, errlen, "%s: record %lld: a score column of %d bytes, outside the [0, %d] of text_width: nothing written", who,
				( long long )h, len, pc.text_width );
			return 1;
		}
		rma::hitct_refusal( err, errlen, who, code, ( long long )h );
		return 1;
	}
	*total = int64_t( s->h_bad[ rma::HBH_TOTAL ] );
	return 0;
}

}	// namespace

extern "C" int rma_hit_ct_size( rma_scanner_t *sc, const rma_db_t *db, const rma_names_t *names, const int32_t *d_hits, int64_t n_hits,
	const uint8_t *d_accept, const uint8_t *d_text_bytes, int32_t text_width, const int32_t *d_text_len, int32_t type, const char *descr_words,
	const uint8_t *letters, int64_t *total, void *stream, char *err, size_t errlen )
{
	const char	*who = "rma_hit_ct_size";
	if( total == nullptr ){
		snprintf( err, errlen, "%s: no room for the total", who );
		return 1;
	}
	*total = 0;
	CtCall	c{ PrintCall{ sc, db, const_cast<rma_names_t *>( names ), d_hits, n_hits, d_accept, d_text_len, text_width }, d_text_bytes, type, {} };
	if( hit_ct_args( who, &c, descr_words, letters, err, errlen ) )
		return 1;
	return n_hits == 0 ? 0 : hit_ct_count( who, c, stream, total, err, errlen );
}

extern "C" int rma_hit_ct( rma_scanner_t *sc, const rma_db_t *db, const rma_names_t *names, const int32_t *d_hits, int64_t n_hits,
	const uint8_t *d_accept, const uint8_t *d_text_bytes, int32_t text_width, const int32_t *d_text_len, int32_t type, const char *descr_words,
	const uint8_t *letters, int64_t total, uint8_t *d_out, int64_t *d_off, void *stream, char *err, size_t errlen )
{
	const char	*who = "rma_hit_ct";
	CtCall	c{ PrintCall{ sc, db, const_cast<rma_names_t *>( names ), d_hits, n_hits, d_accept, d_text_len, text_width }, d_text_bytes, type, {} };
	if( hit_ct_args( who, &c, descr_words, letters, err, errlen ) )
		return 1;
	if( total < 0 || total > INT64_MAX / 16 || d_off == nullptr || ( total > 0 && d_out == nullptr ) ){
		snprintf( err, errlen, "%s: %lld bytes: bad arguments", who, ( long long )total );
		return 1;
	}
	// the outputs: the caller's, each inside its allocation on the scanner's device
	if( rma::check_device_bytes( d_off, sc->device, 0, ( n_hits + 1 ) * 8, "the offsets", err, errlen ) ||
		( total > 0 && rma::check_device_bytes( d_out, sc->device, 0, total, "the .ct bytes", err, errlen ) ) )
		return 1;
	hipStream_t	caller = static_cast<hipStream_t>( stream );
	int64_t	found = 0;
	const uint8_t	*tab = nullptr;
	int	codes = 0;
	// the letters as rma_hit_print takes them, on their way ahead of the count, whose synchronisation leaves the
	// page-locked copy free for the next call
	if( n_hits > 0 && ( letters_on_device( sc->post->win, db, letters, &tab, &codes, err, errlen ) ||
		hit_ct_count( who, c, stream, &found, err, errlen ) ) )
		return 1;
	if( found != total ){
		snprintf( err, errlen, "%s: the .ct records of the %lld records have %lld bytes, not the %lld of `total`: nothing written", who,
			( long long )n_hits, ( long long )found, ( long long )total );
		return 1;
	}
	if( n_hits == 0 ){
		HIPCHK( hipMemsetAsync( d_off, 0, sizeof( int64_t ), caller ) );
		return 0;
	}
	rma::HitPost	&p = *sc->post;
	rma::HitWindowScratch	*s = p.win;
	hipStream_t	st = s->stream.get();
	HIPCHK( hipMemsetAsync( p.hs_carry(), 0, sizeof( int64_t ), st ) );
	for( int64_t c0 = 0; c0 < n_hits; c0 += HW_CHUNK ){
		const int64_t	cn = std::min( HW_CHUNK, n_hits - c0 );
		// (a call of one chunk: the count's offsets are still there)
		if( n_hits > HW_CHUNK && hit_ct_sizes_of( c, c0, cn, s->d_bad + rma::HB_CT_SPARE, err, errlen ) )
			return 1;
		HIPCHK( rma::hit_ct_fill( ct_batch( c, c0, cn ), db->text, tab, codes, s->d_off, p.hs_carry(), d_out, d_off + c0, c0 + cn == n_hits, st ) );
		HIPCHK( rma::hit_carry_add( p.hs_carry(), s->d_off + cn, st ) );
	}
	HIPCHK( hipEventRecord( names->used.get(), st ) );
	return rma::stream_after( caller, st, err, errlen );
}
