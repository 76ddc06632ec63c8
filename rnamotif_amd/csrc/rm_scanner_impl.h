// rm_scanner_impl.h -- the scanner's side (rm_scanner.cpp) as the other host files behind the C ABI see it:
// rm_hitpost.cpp (the consumers of hit records on the device) and rm_gather.cpp (the exchange).  The definitions of
// rma_scanner and rma_db, the few helpers those files call, and the carver of scratch blocks.  No interface: nothing
// outside csrc/ includes it but the host check of the carved layouts (tests/hostsim/carve_check.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "rm_hip_own.h"
#include "rm_flight_count.h"
#include "rm_launch_plan.h"
#include "rm_tail_plan.h"
#include "rm_hitsort.h"
#include "rm_hitsort_dev.h"
#include "rnamotif_amd.h"

#define HIPCHK( call )	do{ hipError_t e_ = ( call ); if( e_ != hipSuccess ){ \
		snprintf( err, errlen, "%s: %s", #call, hipGetErrorString( e_ ) ); return 1; } }while( 0 )

inline size_t align256( size_t x ) { return ( x + 255 ) & ~size_t( 255 ); }

// Arrays one behind the other in a block, each on a 256-byte boundary: take() gives the next one's place from `base`
// and moves on; `at` is then the room taken so far.  From a null base the places are the offsets: the size of a
// block is learnt by carving it once before it is there.
struct Carver {
	size_t	at = 0;
	template<class T> T *take( void *base, size_t count )
	{
		T	*p = reinterpret_cast<T *>( reinterpret_cast<uintptr_t>( base ) + at );
		at += align256( count * sizeof( T ) );
		return p;
	}
};

namespace rma {

struct Block {			// device memory of a device's block cache (DevCtx)
	void	*p = nullptr;
	size_t	bytes = 0;
};
struct DevCtx;			// rm_scanner.cpp: the upload stream and the block cache of one GPU
struct Layout;			// rm_scanner.cpp: the tiling of a database for one launch shape
struct HitPost;			// rm_hitpost.cpp: what its calls keep on the device between them, made on first use
void	hitpost_free( HitPost *p );	// (null: nothing; the scanner's device is current)

// rm_scanner.cpp.  p is device memory of `device` and bytes [lo, hi) from it lie inside its allocation; the caller's
// stream has reached this point before anything later on `on` runs; db is a database rma_db_create_device() or
// rma_db_create_device_fasta() made that has not been destroyed.
int	check_device_bytes( const void *p, int device, int64_t lo, int64_t hi, const char *what, char *err, size_t errlen );
int	stream_after( hipStream_t on, hipStream_t caller, char *err, size_t errlen );
bool	is_device_db( const rma_db *db );
// the upload stream of the database's device, on which db->ready was recorded
hipStream_t	upload_stream( const rma_db *db );
// efn()'s tables on the scanner's device (current), in the buffers that are there when they are large enough
int	efn_tables_to_device( rma_scanner *sc, const rma_efndata_t *efn, char *err, size_t errlen );

}	// namespace rma

// Who frees what, and when.  Device memory, page-locked memory, streams and events are members of the types of
// rm_hip_own.h and go with their holder, in reverse order of declaration; no holder keeps a list of them.  What the
// owners cannot know is the holder's to do first: a destroy function (rma_scanner_destroy, rma_db_destroy,
// rma::hitpost_free, rma::hitwin_scratch_free, rma_comm_destroy) makes the holder's device current, ends what is in
// flight and waits for every stream and event whose work may touch the holder's memory -- and only then deletes.
// A set-up of several pieces (a first use, a regrow) is built in locals and moved into the holder when it is complete:
// a failure leaves the holder as it was, and a capacity is never kept apart from the pointer it describes.
struct rma_scanner {
	rma_program_t	prog;
	rmd_program_t	dprog;
	rma::Options	opt;
	rma::ProgramPlan	plan;		// tile sizes of the descriptor (rma_scanner_create)
	int	device = 0;
	rma::DevCtx	*ctx = nullptr;
	rma::Stream	stream;
	rma::Event	ev[ 5 ];		// search kernel's start / end, efn kernel's, [4]: the search kernel's end when a drain kernel follows
	bool	drained = false;		// the last launch had a drain kernel
	bool	searched = false, efn_ran = false;	// a search kernel was launched at all; the last scan had an efn kernel
	rma::DevMem	d_efn2;			// efn2() tables (rma_efn2data_t), global memory
	bool	need_efn2 = false;
	rma::DevMem	d_prog;			// compact image (rmd_program_t), prog_bytes long
	int	prog_bytes = 0;
	rma::DevMem	d_t16, d_tlkey, d_loginc;	// efn() tables: int16_t, int32_t, int32_t
	bool	have_efn = false;
	rma::DevMem	d_hits;			// [hit_cap()][hit_stride]
	rma::DevMem	d_counters;		// unsigned long long [RMK_N_COUNTERS], rm_diag.h: RMK_C_*
	rma::DevMem	d_spill;		// unsigned [spill_blocks][spill_cap()] queue overflow of every workgroup
	bool	whole_items = false;		// ... which takes the items whole, not in pieces (see search_finish)
	int	glist_cap = 0;			// pooled instance: items of the list the drain kernel walks (the head of d_pool)
	int	glist_need = 0;			// ... and what a scan of the instance that walks nothing asked for (search_finish)
	rma::DevMem	d_pool;			// unsigned [glist_cap + grid_blocks * pool_cap][3] pooled instance: items waiting for pass B
	int	pool_cap = 0;
	rma::PinMem	h_raw;			// int32_t [h_raw_cap()]
	std::vector<int32_t>	h_sorted;
	std::vector<rma::HitKey>	keys, keys_tmp;
	rma::DevHitSort	dsort;		// ordering on the device (rm_hitsort_dev.h)
	rma::PinMem	h_ctr;			// unsigned long long: the first RMK_C_COPIED counters as a launch leaves them, then the word of TAIL_FLAG
	// The word of the counter block in which the ordering of a tail enqueued ahead raises its flag (rm_tail_plan.h): the first
	// one behind those the host reads after every launch, so that one copy brings the count, the repeat conditions and the
	// flag; zeroed with the block before every launch.
	static constexpr int	TAIL_FLAG = RMK_C_COPIED;
	static_assert( TAIL_FLAG < RMK_N_COUNTERS, "a word of the counter block" );
	int	grid_blocks = 0;		// most workgroups of a launch of a lean instance (eight of four waves per CU)
	int	spill_blocks = 0;		// workgroups d_spill has areas for
	// the capacities of d_hits (records), d_spill (items a workgroup) and h_raw (words) are what the buffers hold
	int64_t	hit_cap() const { return int64_t( d_hits.bytes() / ( size_t( dprog.hit_stride ) * sizeof( int32_t ) ) ); }
	int	spill_cap() const { return spill_blocks > 0 ? int( d_spill.bytes() / ( size_t( spill_blocks ) * sizeof( unsigned ) ) ) : 0; }
	size_t	h_raw_cap() const { return h_raw.bytes() / sizeof( int32_t ); }
	// ... and the buffers by the type of what they hold
	int32_t	*hits() const { return d_hits.as<int32_t>(); }
	int32_t	*raw() const { return h_raw.as<int32_t>(); }
	unsigned long long	*counters() const { return d_counters.as<unsigned long long>(); }
	unsigned long long	*ctr() const { return h_ctr.as<unsigned long long>(); }
	const rma_efn2data_t	*efn2() const { return d_efn2.as<rma_efn2data_t>(); }	// (null: none were given)
	// the scan between rma_scan_begin() and rma_scan_end()
	struct InFlight {
		const rma_db	*db = nullptr;
		const rma::Layout	*lay = nullptr;
		rma::LaunchPlan	plan;
		rma::TailPlan	tail;		// energies, ordering and copy back enqueued behind the kernels of rma_scan_begin (rm_tail_plan.h)
	}	fly;
	int64_t	count_max = -1;		// rma::tail_seen() over the counts of the scans this scanner has ended (-1: it has ended none): plan_tail
	int	end_waits = 0, search_launches = 0, efn_launches = 0;	// of the scan begun last, and whether rma_scan_end took
	bool	tail_taken = false;		// the records of the tail enqueued ahead (rma_scanner_last_end)
	rma::FlightMark	flying;			// ... counted among its device's scans in flight (rm_flight_count.h), from its launch to scan_done()
	int	last_launch[ 4 ] = { 0, 0, 0, 0 };	// grid, dynamic LDS, the drain kernel's grid and beside of the last search launch (rma_scanner_last_launch)
	// what the last scan left on the device, in order (rma_scan_end): for rma_gather_hits()
	const int32_t	*d_last = nullptr;
	int64_t	n_last = 0;
	int	last_state = 0;			// where the last scan's ordered records are: 0 no scan has ended, 1 in HBM (d_last; also a scan without records), 2 on the host only
	bool	last_relabelled = false;	// rma_gather_hits has put database-wide entry numbers into d_last's records
	rma::HitPost	*post = nullptr;	// rma_hit_structures, rma_hit_alignment, rma_prune_hits (rm_hitpost.cpp)
};

// a number no other database of the process has had: what outlives a database (a table of its entries' names) knows it
// by this, not by an address the next database may be given
inline uint64_t next_db_serial()
{
	static std::atomic<uint64_t>	last{ 0 };
	return ++last;
}

struct rma_db {
	const uint64_t	serial = next_db_serial();
	int	device = 0;
	rma::DevCtx	*ctx = nullptr;
	rma::Block	blk;			// codes | amask | base_off | slen | pos_lo | pos_hi
	uint32_t	*d_codes = nullptr, *d_amask = nullptr;
	int64_t	*d_base_off = nullptr;
	int32_t	*d_slen = nullptr, *d_pos_lo = nullptr, *d_pos_hi = nullptr;
	std::vector<int32_t>	h_slen, h_pos_lo, h_pos_hi;	// (host copies: the tilings are made from them)
	std::vector<int64_t>	h_base_off;
	std::vector<int64_t>	h_text_start;		// (rma_db_create_device: what the copies to the device read)
	std::vector<uint8_t>	h_table;
	// rma_db_create_device: the text (bytes [text_lo, text_hi) of it hold the entries), the entries' starts and
	// the table on the device, and whether the table was the default one -- what rma_replay_device() reads
	const uint8_t	*text = nullptr;
	int64_t	text_bytes = 0, text_lo = 0, text_hi = 0;
	const int64_t	*d_text_start = nullptr;
	const uint8_t	*d_table = nullptr;
	bool	default_table = true;
	// rma_db_create_device_fasta: the clean text is the database's own, and the entries have names
	// rma_db_text_attach: the same for a database of packed words -- text_blk holds the text made from them (rm_dbtext.h)
	// and, behind it, d_text_start; text_fill_ms is what the fill kernel took
	rma::Block	text_blk;
	float	text_fill_ms = -1.0f;
	std::vector<std::string>	sids, sdefs;
	int32_t	n_seq = 0, max_slen = 0;
	int64_t	total_bases = 0, sum_slen = 0;
	int64_t	padded_bases = 0;	// bases the packed arrays hold, padding between the entries included
	bool	ascending = true;	// the entries lie in the packed arrays in their order, none overlapping
	rma::Event	ready;			// the upload is complete (recorded on the upload stream)
	std::mutex	mu;			// layouts, busy
	std::vector<std::unique_ptr<rma::Layout>>	layouts;	// (made and destroyed in rm_scanner.cpp alone)
	std::vector<rma_scanner *>	busy;		// scanners with a scan of this database in flight
};
