/*
 * rnamotif_amd.h -- C ABI of the MI355X scan path.
 *
 * The reference has no plug-in API; the boundary this library replaces is the
 * set of calls main() makes around the scan (/root/reference/src/rnamot.c:49-188,
 * prototypes in /root/reference/src/rnamot.h:305-381):
 *
 *   RM_init() + yyparse() + SE_link() + RM_linkscore()   -> rma_descr_compile()
 *   RM_fm_init()                  (find_motif.c:109)      -> rma_scanner_create()
 *   FN_fgetseq() into sbuf        (dbutil.c:42)           -> rma_db_create()
 *   RM_find_motif() x2 per entry  (find_motif.c:164)      -> rma_scan()
 *   RM_score() + print_match()    (score.c:608,
 *                                  find_motif.c:1826)     -> rma_replay_*()
 *
 * Plain C: pointers, sizes, integer status codes.  Every function that can
 * fail returns 0 on success and non-zero with a message in err[] otherwise;
 * nothing in the library calls exit().  The scan runs on the GPU only: there is
 * no CPU fallback, rma_scanner_create() fails when no HIP device is usable.
 */
#ifndef RNAMOTIF_AMD_H
#define RNAMOTIF_AMD_H

#include <stddef.h>
#include <stdint.h>
#include "rnamotif_amd_program.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rma_descr	rma_descr_t;	/* compiled descriptor + score program (host)	*/
typedef struct rma_scanner	rma_scanner_t;	/* motif program + buffers on one GPU		*/
typedef struct rma_db		rma_db_t;	/* packed sequences resident in HBM		*/
typedef struct rma_score	rma_score_t;	/* a score section's MAIN as an image for the device	*/
typedef struct rma_replay	rma_replay_t;	/* score VM + hit printer state			*/

const char	*rma_version( void );
int	rma_device_count( void );

/* ---- descriptor front end (host).  argv is the rnamotif command line
 * (argv[0] = program name, "-descr file", "-Dname=value", "-sh", "-context", ...);
 * database file names in it are remembered for rma_descr_dbfiles(). */
int	rma_descr_compile( int argc, const char *const *argv, rma_descr_t **out, char *err, size_t errlen );
void	rma_descr_free( rma_descr_t *d );
const rma_program_t	*rma_descr_program( const rma_descr_t *d );
const rma_efndata_t	*rma_descr_efndata( const rma_descr_t *d );	/* NULL: no efn() in the score section */
const rma_efn2data_t	*rma_descr_efn2data( const rma_descr_t *d );	/* NULL: no efn2() in the score section */
int	rma_descr_minlen( const rma_descr_t *d );			/* rm_dminlen */
int	rma_descr_maxlen( const rma_descr_t *d );			/* rm_dmaxlen, RMA_UNBOUNDED if open */
/* the fields of the "#RM descr" line the printer writes for this descriptor, one per printed column, separated by
 * blanks (e.g. "h5(tag='1') ss h3(tag='1')"), into buf (NUL-terminated, cut at buflen); returns their length */
size_t	rma_descr_names( const rma_descr_t *d, char *buf, size_t buflen );
/* for bindings that do not want to mirror the struct: n_elems, n_searches, hit stride,
 * ctx offset, efn offset, n_efn_sites, chk_both_strs, windowsize */
void	rma_program_info( const rma_program_t *prog, int32_t info[ 8 ] );
/* the number of elements whose seq= the scan tests loosely (rma_regex_t::loose: back references, letters that
 * are not acgt with iupac = 0): a scan's records of such a program are a superset of the reference's candidates
 * until they are replayed (rma_replay_*), which applies the whole expression to the text */
int	rma_program_loose( const rma_program_t *prog );

/* ---- energy tables on their own: RM_getefndata() efn.c:157 / RM_getefn2data() efn2.c:130
 * from the directory dir (the reference's efn_datadir / $EFNDATA). */
int	rma_efndata_load( const char *dir, rma_efndata_t *out, char *err, size_t errlen );
int	rma_efn2data_load( const char *dir, rma_efn2data_t *out, char *err, size_t errlen );

/* ---- scanner.  prog (and efn, may be NULL) are copied. */
int	rma_scanner_create( const rma_program_t *prog, const rma_efndata_t *efn, int device,
		rma_scanner_t **out, char *err, size_t errlen );
/* tables for the program's efn2() sites (RM_getefn2data, efn2.c:130); copied to the device */
int	rma_scanner_set_efn2data( rma_scanner_t *sc, const rma_efn2data_t *efn2, char *err, size_t errlen );
/* Launch-shape and diagnostic switches (DESIGN.md has the table).  The RNAMOTIF_* environment is read
 * once, by rma_scanner_create(); the switches that may change between scans change through this call
 * only: "dbg", "pool", "pool_min", "pool_refill", "drain", "glist", "drain_waves", "search_wgs", "struct_wgs", "score_budget", "score_heap", "flush", "efn_light", "host_sort", "spec_tail", "timing", "short".
 * None of them changes the records a scan returns. */
int	rma_scanner_set_option( rma_scanner_t *sc, const char *name, int value, char *err, size_t errlen );
/* One scan of eight start positions, thrown away: what the runtime sets up on first use (code objects,
 * the first allocations, the ordering's kernels) is paid here and not in the first batch of a search.
 * The command line program calls it once the scanner is complete; the library never does by itself. */
int	rma_scanner_warmup( rma_scanner_t *sc, char *err, size_t errlen );
void	rma_scanner_destroy( rma_scanner_t *sc );

/* ---- database: n sequences of lower case letters as the reference's readers
 * deliver them (dbutil.c: every alpha character kept, u -> t).  They are packed
 * 2 bits + 1 ambiguity bit per base and uploaded; the host text is not kept.  A database
 * lives on the device of the scanner named at its creation (sc may be NULL: device 0) and holds
 * nothing that depends on a descriptor: every scanner of that device can scan it, side by side if
 * they like (rma_db_attach, rma_scan_begin) -- one upload, many descriptors.  Device memory of a
 * destroyed database is kept for the next one of about its size (no allocation per batch). */
int	rma_db_create( rma_scanner_t *sc, const char *const *seqs, const int32_t *slens, int32_t n,
		rma_db_t **out, char *err, size_t errlen );
/* The same, answering only for start positions pos_lo[i] <= szero < pos_hi[i] of each strand
 * of entry i (RM_find_motif's szero, find_motif.c:184-205): a long entry can be searched by
 * several devices, each holding the whole entry and a slice of its start positions; the union
 * of the hit records, sorted by their first five words, is the whole entry's hit list. */
int	rma_db_create_ranges( rma_scanner_t *sc, const char *const *seqs, const int32_t *slens,
		const int32_t *pos_lo, const int32_t *pos_hi, int32_t n,
		rma_db_t **out, char *err, size_t errlen );
void	rma_db_destroy( rma_db_t *db );
int64_t	rma_db_bases( const rma_db_t *db );
/* Lay db out for scanner sc (the tiling of its entries for that descriptor's tile size) ahead of sc's
 * first scan of it, which would otherwise do it.  A database may be attached to any number of scanners
 * of its device. */
int	rma_db_attach( rma_scanner_t *sc, rma_db_t *db, char *err, size_t errlen );
/* wait until the upload of db is complete (rma_db_create_packed_async) */
int	rma_db_wait( rma_db_t *db, char *err, size_t errlen );

/* ---- packed database on disk (no counterpart in the reference, which re-reads the text
 * on every run, rnamot.c:157-183): the readers' output -- names, definition lines and
 * sequences as FN_/PIR_/GB_fgetseq deliver them (dbutil.c:42,130,226) -- stored in the
 * layout rma_db_create() makes, plus the letters at ambiguous positions, so that a scan
 * can start from it directly and print_match()'s text can still be rebuilt. */
typedef struct rma_pack	rma_pack_t;
int	rma_pack_write( const char *path, const char *const *sids, const char *const *sdefs,
		const char *const *seqs, const int32_t *slens, int32_t n, char *err, size_t errlen );
int	rma_pack_open( const char *path, rma_pack_t **out, char *err, size_t errlen );
void	rma_pack_close( rma_pack_t *pk );
int32_t	rma_pack_count( const rma_pack_t *pk );
int64_t	rma_pack_bases( const rma_pack_t *pk );
const char	*rma_pack_sid( const rma_pack_t *pk, int32_t i );
const char	*rma_pack_sdef( const rma_pack_t *pk, int32_t i );
int32_t	rma_pack_slen( const rma_pack_t *pk, int32_t i );
/* buf must hold rma_pack_slen( pk, i ) + 1 bytes */
int	rma_pack_seq( const rma_pack_t *pk, int32_t i, char *buf );
/* entries [first, first+count) straight into HBM; hit records count entries from first */
int	rma_db_create_packed( rma_scanner_t *sc, const rma_pack_t *pk, int32_t first, int32_t count,
		rma_db_t **out, char *err, size_t errlen );
/* The same without waiting for the copies: they run on the device's upload stream, under whatever the
 * scanners' streams are doing; a scan of the database waits for them on the device.  The pack must
 * stay as it is until rma_db_wait() or the end of a scan of the database.  From page-locked memory
 * (rma_pack_pin) the call returns at once; from pageable memory the runtime stages the words first. */
int	rma_db_create_packed_async( rma_scanner_t *sc, const rma_pack_t *pk, int32_t first, int32_t count,
		rma_db_t **out, char *err, size_t errlen );
/* page-lock the packed words of pk so that uploads from it are plain DMA (undone by rma_pack_close) */
int	rma_pack_pin( rma_pack_t *pk, char *err, size_t errlen );
/* The same database in memory, read from sequence files the way rnamotif reads them (DB_fnext,
 * dbutil.c:12-40; fmt "fastn" | "pir" | "gb" or NULL; maxslen = rnamotif's -N, 0 for its default):
 * FASTA files through the parallel reader, everything else -- and every entry a reader has a
 * diagnostic for -- through the restatements of FN_/PIR_/GB_fgetseq, which print what the
 * reference prints.  Files that are packed databases already are appended as they are. */
int	rma_pack_read( const char *const *paths, int32_t n_paths, const char *fmt, int32_t maxslen, int32_t threads,
		rma_pack_t **out, char *err, size_t errlen );
/* A rank's share of a database without reading the rest (one process per GPU).
 * rma_database_index(): the entries of the files in order and an upper bound of each one's length --
 * its bytes in a FASTA file ('>' found by all threads, nothing parsed), its length in a packed
 * database -- for the ranks to divide among themselves; *extent is to be released with rma_free().
 * rma_pack_read_entries(): the entries with the given numbers (ascending), read and packed; the
 * other entries' bytes are not touched.  Both return 2, with nothing made, when the files can only be
 * read whole -- -fmt pir | gb, a file that cannot be mapped, an entry the serial reader has a
 * diagnostic for: the caller then reads everything with rma_pack_read(). */
int	rma_database_index( const char *const *paths, int32_t n_paths, const char *fmt, int32_t threads,
		int64_t **extent, int32_t *n_entries, char *err, size_t errlen );
int	rma_pack_read_entries( const char *const *paths, int32_t n_paths, const char *fmt, int32_t maxslen, int32_t threads,
		const int32_t *entry, int32_t n, rma_pack_t **out, char *err, size_t errlen );
void	rma_free( void *p );
/* Any n entries of a packed database, entry[i] with start positions pos_lo[i] <= szero < pos_hi[i]
 * (NULL: all), straight into HBM: what one rank of a multi-GPU search takes of a database every
 * rank has read.  Hit records number the entries 0 .. n-1 in the order given. */
int	rma_db_create_packed_ranges( rma_scanner_t *sc, const rma_pack_t *pk, const int32_t *entry,
		const int32_t *pos_lo, const int32_t *pos_hi, int32_t n, rma_db_t **out, char *err, size_t errlen );

/* ---- databases from text already in device memory.  Entry i is the slen[i] bytes at text + start[i]
 * (start, slen, pos_lo, pos_hi are host arrays; pos_lo/pos_hi may be NULL, else as rma_db_create_ranges),
 * all inside the text_bytes bytes at text, which is memory of the scanner's device.  The words are the
 * ones rma_db_create() makes of the same bytes, packed by a kernel on the device's upload stream.
 * table: NULL = the readers' letters (acgtu in either case, every other byte ambiguous), else 256 codes,
 * byte -> 0-3 or 4 (ambiguous), in host memory or on the scanner's device (there a code above 3 counts as
 * 4).  stream: the caller's hipStream_t the text was written on (NULL = the default stream): the packing
 * runs behind what is queued there now.  The text stays as it is, and allocated, until rma_db_wait()
 * returns or a scan of the database has ended, and, to replay (rma_replay_device), until the replay
 * returns.  Pointers are checked (device memory of the scanner's
 * device, ranges inside the text and its allocation) before anything is launched. */
int	rma_db_create_device( rma_scanner_t *sc, const void *text, int64_t text_bytes, const int64_t *start, const int32_t *slen,
		const int32_t *pos_lo, const int32_t *pos_hi, int32_t n, const uint8_t *table, void *stream,
		rma_db_t **out, char *err, size_t errlen );
/* A database of FASTA text in device memory: text_bytes bytes as a file holds them -- '>' lines, line breaks,
 * digits, blanks.  The entries and their letters are found on the device as the readers find them (FN_fgetseq:
 * an entry starts at a '>' outside a definition line, its letters are the isalpha() bytes up to the next start)
 * and written to a clean text the database owns: 1 byte per base of device memory until rma_db_destroy(), which
 * returns it to the cache.  From there on it is a rma_db_create_device() database of the readers' letters over
 * that text (rma_replay_device works on it).  maxslen as rma_pack_read (0 = the readers' default).  The work
 * runs on the device's upload stream behind what is queued on `stream` now.  Unlike rma_db_create_device this
 * call synchronises -- it learns the number of entries and letters before it can allocate, and the definition
 * lines before it can return; in return the caller's text is no longer needed once it has returned.  Refused,
 * with the entry's number, the byte offset of its '>' and the reason, and nothing made: what the parallel reader
 * hands to the serial reader's diagnostics -- text that does not begin with '>', an unnamed entry, a definition
 * line of 19999 bytes or more or with a NUL in it (any line of more than 20256 bytes counts as too long), an
 * entry of more than maxslen letters -- and more than INT32_MAX entries.  Empty text is a database of no entries. */
int	rma_db_create_device_fasta( rma_scanner_t *sc, const void *text, int64_t text_bytes, int32_t maxslen,
		void *stream, rma_db_t **out, char *err, size_t errlen );
/* entry i's name and definition as the readers deliver them (the name cut at 99 bytes); valid until rma_db_destroy.
 * Non-zero for a database that was not made by rma_db_create_device_fasta and has had no rma_db_text_attach_pack,
 * or an entry it does not have. */
int	rma_db_entry_name( const rma_db_t *db, int32_t i, const char **sid, const char **sdef );
/* the number of entries of a database */
int32_t	rma_db_entries( const rma_db_t *db );
/* how rma_db_create_device_fasta cuts its text (for tests that place bytes at the seams): shape[ 0 ] bytes per
 * chunk, counted from the aligned dword the text begins in; shape[ 1 ] chunks per block of the scan; shape[ 2 ]
 * bytes of a definition line that are looked at */
void	rma_fasta_device_shape( int32_t shape[ 3 ] );
/* the default table of rma_db_create_device: byte -> code (0-3) or 4, the readers' letters */
void	rma_letter_codes( uint8_t codes[ 256 ] );
/* a database's packed words read back (for verification; whichever path made them): codes[ 2 * w ],
 * amask[ w ] with w = rma_db_mask_words( db ), base_off[ n ], slen[ n ]; any of them may be NULL */
int64_t	rma_db_mask_words( const rma_db_t *db );
int	rma_db_read_packed( const rma_db_t *db, uint32_t *codes, uint32_t *amask, int64_t *base_off, int32_t *slen,
		char *err, size_t errlen );
/* The text of a database of packed words (rma_db_create*(), rma_db_create_packed*()), made on the device from the
 * words in HBM (csrc/rm_dbtext.h has the rule, PackFile::unpack's): 1 byte per base of device memory, each entry on a
 * 16-byte boundary, until rma_db_destroy(), which returns it to the cache.  From then on the database is a
 * rma_db_create_device() database of the readers' letters over that text: rma_replay_device() and every call over
 * hit records on the device work on it.  Its words, tilings and scans are unchanged.
 * exc: the letters at masked positions, entry after entry, in order; exc_off[ n_seq + 1 ] (host arrays).
 * exc NULL: every masked base reads n.
 * The call orders itself behind `stream` and the database's upload, and waits once.  Refused, with words, nothing made
 * and the database as it was: a database that has its text already (made from device text, or attached before), one
 * with a scan in flight, a destroyed one, exc_off that does not ascend from 0, an entry whose mask has another number
 * of bases set than it has exceptions, an exception that is not a lower-case letter other than a, c, g and t. */
int	rma_db_text_attach( rma_db_t *db, const char *exc, const int64_t *exc_off, void *stream, char *err, size_t errlen );
/* the same from the pack the database was made of: entry i of db is entry entry[ i ] of pk (entry NULL: first + i).
 * The entries also get the pack's names (rma_db_entry_name).  Refused as well: a pack entry out of range or of
 * another length than the database's. */
int	rma_db_text_attach_pack( rma_db_t *db, const rma_pack_t *pk, const int32_t *entry, int32_t first, void *stream,
		char *err, size_t errlen );
/* verification, like rma_db_read_packed(): entry i's text read back, slen bytes (any database with text on the device) */
int	rma_db_read_text( const rma_db_t *db, int32_t i, char *buf, char *err, size_t errlen );
/* what the fill kernel of rma_db_text_attach*() took on the device, in ms (profiles); negative: never attached */
float	rma_db_text_fill_ms( const rma_db_t *db );

/* ---- scan every sequence of db (both strands when the program says so).
 * *hits receives *n_hits records of rma_hit_stride( prog ) words, sorted by
 * (seq, comp, szero, rank, order) = the reference's output order; the memory
 * belongs to the scanner and is valid until its next scan BEGINS (rma_scan, rma_scan_begin, rma_scan_device) or its
 * destruction: a scanner's next begin may write the same memory, or free it, before that scan's end is called.
 * Energies of the program's efn sites are filled in.  The records are candidates before the score section;
 * for a program with loose seq= elements (rma_program_loose() > 0) they are a superset of the reference's
 * candidates until replayed. */
int	rma_scan( rma_scanner_t *sc, const rma_db_t *db, const int32_t **hits, int64_t *n_hits,
		char *err, size_t errlen );

/* rma_scan() in two halves.  rma_scan_begin() puts the search kernel on the scanner's stream and
 * returns; rma_scan_end() waits for it, runs the energy kernel and the ordering, copies the records
 * back and returns them as rma_scan() does.  Between the two the host is free: to begin the scan of
 * another scanner (two descriptors over one database run side by side), or to upload the next
 * database (rma_db_create_packed_async).  One scan in flight per scanner.  rma_scan_end's records are
 * rma_scan's: a superset of the candidates for a program with loose seq= elements until replayed.
 * Lifetime of *hits: until the SAME scanner's next rma_scan_begin() (not only its next end) -- from its second scan on
 * a scanner's begin enqueues the energies, the ordering and the records' way into that memory behind the kernels
 * (rma_scanner_last_end below), and may replace the memory by a larger piece.  Read or copy a scan's records before
 * beginning that scanner's next scan; another scanner's begin touches nothing of it.  The same holds for *d_hits of
 * rma_scan_end_on_device(). */
int	rma_scan_begin( rma_scanner_t *sc, const rma_db_t *db, char *err, size_t errlen );
int	rma_scan_end( rma_scanner_t *sc, const int32_t **hits, int64_t *n_hits, char *err, size_t errlen );
/* rma_scan_end() that leaves the ordered records in HBM (*d_hits is a device pointer, valid until
 * the scanner's next scan): for rma_gather_hits(), which sends them from there. */
int	rma_scan_end_on_device( rma_scanner_t *sc, const int32_t **d_hits, int64_t *n_hits, char *err, size_t errlen );

/* The last scan's ordered records (left in HBM by rma_scan_end_on_device, or by rma_scan_end when they
 * were ordered on the device) into dst, device memory of the scanner's device with room for dst_words
 * words: the copy is ordered after the scanner's work and before what is queued on `stream` (the caller's
 * hipStream_t, NULL = the default stream) from now on.  dst is checked as rma_db_create_device's text. */
int	rma_scan_records_to_device( rma_scanner_t *sc, int32_t *dst, int64_t dst_words, void *stream, char *err, size_t errlen );

/* The device part of rma_scan() alone (search kernel + efn kernel, no copy back,
 * no sort), for measurement: returns the candidate count and the time of the
 * search kernel as measured with HIP events on the scanner's stream. */
int	rma_scan_device( rma_scanner_t *sc, const rma_db_t *db, int64_t *n_hits, float *search_ms,
		float *efn_ms, char *err, size_t errlen );
/* The kernels of the scanner's last search (HIP events on its stream): ms[0] the search kernel, ms[1] the
 * drain kernel that walked the items the search kernel left in its list (0: the search kernel walked
 * them itself), ms[2] the efn kernel (0: none).  search_ms above is ms[0] + ms[1]. */
int	rma_scanner_last_kernel_ms( rma_scanner_t *sc, float ms[ 3 ], char *err, size_t errlen );
/* The shape of the scanner's last search launch: out[0] workgroups of the search kernel, out[1] bytes of
 * dynamic LDS a workgroup, out[2] workgroups of the drain kernel behind it (0: none), out[3] 1 when the
 * shape was chosen to leave another scanner's drain kernel room on every CU (option "beside": -1, the
 * default, when another scanner of the device has a scan in flight as this one begins; 0 never; 1 always).
 * All 0 before the first launch.  Returns 0. */
int	rma_scanner_last_launch( rma_scanner_t *sc, int out[ 4 ] );
/* What the scanner's last rma_scan_end() (rma_scan(), rma_scan_end_on_device()) did.  From a scanner's second scan on,
 * rma_scan_begin() enqueues the scan's tail -- energies, ordering, the records' way back -- behind its kernels, sized by
 * the scans the scanner has ended; rma_scan_end() then waits once and takes the records, or, when the scan found more
 * than was planned for or has to be repeated, does the tail again as a first scan does.  Option "spec_tail": -1, the
 * default, by that rule; 0 never.  dbg, timing and host_sort turn it off, and rma_scan_device() never does it.
 * out[0] the times the end waited for the scanner's stream, out[1] 1 when it took the records of the tail enqueued
 * ahead, out[2] launches of the search kernel, out[3] launches of an energy kernel, both from the scan's begin.
 * Returns 0. */
int	rma_scanner_last_end( rma_scanner_t *sc, int out[ 4 ] );

/* Records from several scans (the slices of one database searched by several GPUs or hosts, word 0
 * already the database-wide entry number) into the reference's output order: by the five header
 * words, ties in the order given; the order word is renumbered within (entry, strand, start, rank).
 * out[n][stride] must not overlap hits.  Host only -- what rank 0 of mrnamotif does with the
 * MT_RESULT messages it receives (mrnamotif.c:733-760). */
int	rma_sort_hits( const int32_t *hits, int64_t n_hits, int32_t stride, int32_t *out, char *err, size_t errlen );

/* ---- the one exchange of a multi-GPU search: the records of every rank's last scan to one rank,
 * over RCCL (xGMI), device to device -- mrnamotif's MT_RESULT messages, mrnamotif.c:733-760 and
 * :898-917.  One process per GPU.  Rank 0 makes an id (rma_comm_unique_id) and hands it to the
 * others by whatever the job has (MPI_Bcast, a torch.distributed broadcast, a file); every rank then
 * calls rma_comm_create() -- collectively.  RCCL is loaded at run time (librccl.so.1); a world of
 * one rank needs none. */
#define RMA_COMM_ID_BYTES	128
typedef struct rma_comm	rma_comm_t;
int	rma_comm_unique_id( uint8_t id[ RMA_COMM_ID_BYTES ], char *err, size_t errlen );
int	rma_comm_create( const uint8_t id[ RMA_COMM_ID_BYTES ], int rank, int world, int device,
		rma_comm_t **out, char *err, size_t errlen );
void	rma_comm_destroy( rma_comm_t *comm );
/* The collective calls rma_gather_hits() makes, as a table.  rma_comm_create() fills it with RCCL's
 * (ncclAllGather of int64, ncclSend / ncclRecv of int32, ncclGroupStart / ncclGroupEnd, ncclCommCount); a caller
 * with another transport of the same semantics -- MPI between nodes where mrnamotif.c has MPI_Send / MPI_Recv, or
 * a test that makes a call fail -- hands its own to rma_comm_create_on().  Every call returns 0 or a code that
 * error_string() puts into words; stream is the hipStream_t the buffers are valid on; buffers are in HBM. */
typedef struct rma_transport {
	int	( *all_gather )( void *ctx, const void *send, void *recv, size_t n_int64_per_rank, void *stream );
	int	( *send )( void *ctx, const void *buf, size_t n_int32, int peer, void *stream );
	int	( *recv )( void *ctx, void *buf, size_t n_int32, int peer, void *stream );
	int	( *group_start )( void *ctx );
	int	( *group_end )( void *ctx );
	const char	*( *error_string )( void *ctx, int code );	/* may be null */
	int	( *comm_count )( void *ctx, int *count );		/* may be null */
	void	*ctx;
} rma_transport_t;
int	rma_comm_create_on( const rma_transport_t *transport, int rank, int world, int device,
		rma_comm_t **out, char *err, size_t errlen );
/* The number of ranks the transport itself reports (RCCL: ncclCommCount; a world of one: 1). */
int	rma_comm_count( rma_comm_t *comm, int *count, char *err, size_t errlen );
/* Collective.  Every rank has ended a scan of its shard with rma_scan_end_on_device() (or rma_scan_end:
 * the records are still in HBM).  global_index[ i ], i < n_index, is the number in the whole database
 * of entry i of this rank's shard: word 0 of the records is rewritten to it on the device (once per scan: a second
 * gather of the same records leaves them).  An all-gather of the counts and of a flag per rank (16 bytes per rank: a
 * rank that cannot take part -- records ordered on the host, no entry numbers -- says so there, and every rank
 * returns an error instead of waiting), a second one only when the root's buffers have to grow (could they?), then one
 * grouped send/receive, whose group is closed on every path: on rank `root`,
 * *hits / *n_hits are all records, rank by rank, each rank's part in the reference's order (when the
 * ranks hold consecutive runs of entries that is the whole job's order; otherwise rma_sort_hits()
 * merges); elsewhere *n_hits = 0.  counts, if not NULL, receives every rank's count on every rank.
 * The memory belongs to the communicator and is valid until its next gather. */
int	rma_gather_hits( rma_comm_t *comm, rma_scanner_t *sc, const int32_t *global_index, int32_t n_index, int root,
		const int32_t **hits, int64_t *n_hits, int64_t *counts, char *err, size_t errlen );

/* ---- replay: run the score program over candidates and print accepted hits
 * in the reference's format to a stdio stream opened on path ("-" = stdout). */
int	rma_replay_open( rma_descr_t *d, const char *path, rma_replay_t **out, char *err, size_t errlen );
/* one batch: the same sequences (ids, definition lines, text) the db was made from */
int	rma_replay_batch( rma_replay_t *rp, const char *const *sids, const char *const *sdefs,
		const char *const *seqs, const int32_t *slens, int32_t n,
		const int32_t *hits, int64_t n_hits, int64_t *n_printed, char *err, size_t errlen );
/* the same over a packed database: word 0 of a record is the entry's number in pk minus first; the
 * text of an entry is rebuilt for the span of each hit only */
int	rma_replay_pack( rma_replay_t *rp, const rma_pack_t *pk, int32_t first,
		const int32_t *hits, int64_t n_hits, int64_t *n_printed, char *err, size_t errlen );
/* Replay candidates of a database made by rma_db_create_device(): the score program, the loose seq= test and
 * the printer, as rma_replay_batch() runs them, over text read from the database's device text -- of each
 * record only its window, the bases its elements and contexts cover, cut out on the device and copied back.
 * d_hits: n_hits records of rma_hit_stride() words of the replay's program in device memory of the database's
 * device (a subset of a scan's records, in any order; printed in the order given).  letters: 256 bytes,
 * byte -> the letter the replay sees, or NULL: the readers' letters (an ASCII letter in lower case, u as t,
 * every other byte n) for a database made with the default table, else "acgt" for codes 0-3 of its table and
 * n for the rest.  On strand 1 the letters are complemented as mk_rcmp() does (a t, c g, g c, t/u a, else n).
 * sids / sdefs: one per entry, or NULL (sid = the entry's number in decimal, sdef "").  stream: the caller's
 * hipStream_t the records and text were written on (NULL = the default stream).  accepted: host array of
 * n_hits bytes or NULL; 1 where the record was printed (reached the printer: with HOLD, was held).
 * *n_printed = their number.  Every record is checked on the device before any text is read (entry inside
 * the database, strand 0 or 1, every element and context inside its entry); a bad record fails the call,
 * naming its index, and nothing is printed.  The replay's device and page-locked buffers are made on the
 * first call, on the database's device, and freed by rma_replay_close(). */
int	rma_replay_device( rma_replay_t *rp, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
		const uint8_t *letters, const char *const *sids, const char *const *sdefs, void *stream,
		int64_t *n_printed, uint8_t *accepted, char *err, size_t errlen );
int	rma_replay_close( rma_replay_t *rp, char *err, size_t errlen );	/* runs the END program */

/* ---- hit structures as device tensors: the records of a database made by rma_db_create_device() or
 * rma_db_create_device_fasta() expanded base by base, on the device (csrc/rm_hitstruct.h has the rule, shared by
 * the host and the kernel).  The unit is a record's window as rma_replay_device() cuts it: the bases its elements
 * and contexts cover, window h at [ off[ h ], off[ h + 1 ] ) of the per-base arrays, lo[ h ] its first position on
 * the hit's strand.  Per base: base, its letter as rma_replay_device() reads it (letters as there); elem, the
 * descriptor element it belongs to (n_elems / n_elems + 1: the left / right context, -1: none); mate[ 3 ], the
 * window indices of the bases it is matched with in the other strands of its helix, in descriptor order, padded
 * with -1 -- one for h5/h3 and p5/p3, two for a triplex, three for a 4-plex, whether or not the matcher counted
 * the position as a mispair.  d_hits: n_hits records of the scanner's program in memory of its device, any rows
 * in any order.  Every record is checked on the device before anything is written: rma_replay_device()'s checks,
 * and the strands of a helix having one length; a bad record fails the call, naming its index.
 * rma_hit_structures_size() returns the window bytes of all records in *total and synchronises once.
 * rma_hit_structures() checks and counts again (it keeps nothing from the first call; one wait for two words),
 * refuses a total that is not what it finds, then queues the kernels that fill the outputs and returns without
 * waiting for them: they run behind what is queued on `stream` (the caller's hipStream_t, NULL = the default
 * stream) now and ahead of what is queued there next.  The outputs are device memory of the scanner's device,
 * checked as rma_db_create_device's text.  Scratch is the scanner's, made on the first call. */
int	rma_hit_structures_size( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
		void *stream, int64_t *total, char *err, size_t errlen );
int	rma_hit_structures( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
		const uint8_t *letters, int64_t total,
		int64_t *d_off /* n_hits+1 */, int32_t *d_lo /* n_hits */, uint8_t *d_base /* total */,
		int16_t *d_elem /* total */, int32_t *d_mate /* 3*total */,
		void *stream, char *err, size_t errlen );

/* ---- hit records as an alignment, on the device: the byte matrix whose row h, cut into lines of 70 bytes, is what
 * `rmfmt -a` writes as the sequence lines of record h's printed form (csrc/rm_hitalign.h has the rule, shared by the
 * host and the kernels).  Columns stand in the order the fields are printed: the left context when the descriptor
 * has one, the elements, the right context when it has one (at most 102).  A field is as wide as it is printed (an
 * empty element 1, the "."); a column as wide as its widest field over the records given; h3, t2, q2 and q4 columns
 * are right-aligned, all others left-aligned.  A row has W = sum of the widths + n_cols - 1 bytes: every field padded
 * to its column's width with the gap byte, one separator byte between columns.  The letters are those of
 * rma_hit_structures() (letters as there).  d_pos, where given, receives for every letter byte the position on the
 * hit's strand it came from (the coordinate of rma_hit_structures' lo), -1 for every other byte.  d_hits: n_hits
 * records of the scanner's program in memory of its device, any rows in any order; pointers are checked as
 * rma_hit_structures checks them.  Every record is checked on the device first (rma_replay_device()'s checks; strands
 * of unequal length are not refused, as rmfmt does not refuse them); a bad record fails the call, naming its index.
 * rma_hit_alignment_shape() checks the records, reduces the widths and waits once: *n_cols, widths[ c ] for
 * c < *n_cols (0 behind them), right[ c ] = 1 for a right-aligned column, *row_bytes = W.  With n_hits == 0 the widths
 * are 0 and *row_bytes is n_cols - 1.
 * rma_hit_alignment() checks and reduces again (it keeps nothing from the first call; one wait), refuses a bad record
 * and any given width below what the records need, naming the column, then queues the fill and returns without
 * waiting for it: it runs behind what is queued on `stream` (the caller's hipStream_t, NULL = the default stream) now
 * and ahead of what is queued there next.  Given widths may be larger than needed: that is how several batches share
 * one set of columns.  fill: the gap, separator and empty-field bytes, NULL for rmfmt's "-|.".  n_hits == 0 writes
 * nothing.  Scratch is the scanner's, made on the first call and freed by rma_scanner_destroy(). */
int	rma_hit_alignment_shape( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
		int32_t *n_cols, int32_t *widths /* host, room for 102 */, uint8_t *right /* host, 102, may be NULL */,
		int64_t *row_bytes, void *stream, char *err, size_t errlen );
int	rma_hit_alignment( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
		const int32_t *widths /* host, n_cols */, const uint8_t *letters /* 256 or NULL */,
		const uint8_t fill[ 3 ] /* gap, separator, empty; NULL: "-|." */,
		uint8_t *d_rows /* n_hits * W */, int32_t *d_pos /* n_hits * W or NULL */,
		void *stream, char *err, size_t errlen );

/* ---- rmprune's rule over records, on the device: d_keep[ h ] = 1 where the rmprune tool would keep record h of the
 * n_hits records at d_hits, 0 where it would drop it as an "unzipped" version of another -- the decisions the tool
 * makes on the printed form of the same records in the same order (csrc/rm_prune.h has the rule, shared by the host
 * and the kernels; csrc/tools/rmprune.cpp is the tool).  In a paragraph: consecutive records whose entries have
 * the same name group are a run, cut into blocks of 1000; inside a block the records in front of the first one on
 * strand 1 and those from it on are split into groups, a new group wherever a record leaves the span of its group's
 * first record; inside a group of two or more every kept record b, from the last to the second, is compared with
 * the kept records b1 in front of it, nearest first, by the printed spans of their helix strands: where b1 is b
 * with base pairs opened at the inside end of helices b1 is dropped, where b is b1 so unzipped b is dropped and its
 * pass ends.  db: any database of the scanner's device; only its entry lengths are read, no text is needed.
 * group_of_entry: host array of one id per entry of db, equal ids for entries the tool takes as one name (a sid up
 * to its first '.' or blank), or NULL: every entry its own.  d_hits / d_keep: device memory of the scanner's
 * device, checked as rma_hit_structures checks its outputs; any rows in any order, and the order given is the order
 * judged.  Every record is checked on the device first (rma_replay_device()'s checks); a bad record fails the call,
 * naming its index, and d_keep is not written.  n_hits == 0 does nothing.  The kernels are queued on `stream` (the
 * caller's hipStream_t, NULL = the default stream); the call waits once, for the check's result and the number of
 * blocks, then queues the last kernel and returns without waiting for it.  Scratch (16 + 8 bytes per helix strand
 * + 9 bytes per record) is the scanner's, made on the first call and grown. */
int	rma_prune_hits( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
		const int32_t *group_of_entry /* host, n_seq, or NULL */, uint8_t *d_keep /* n_hits */,
		void *stream, char *err, size_t errlen );

/* ---- energies of structures in device tensors: efn() and efn2() of any batch of structures, as the reference's
 * efn_drv and efn2_drv give them for a .ct file (csrc/rm_structenergy.h has the rule, shared by the host and the
 * kernels).  The tables are the scanner's: a descriptor's own (rma_scanner_create, rma_scanner_set_efn2data), or
 * those rma_scanner_load_energy_tables() reads from dir (rma_efndata_load / rma_efn2data_load; which: 1 efn, 2 efn2,
 * 3 both) and uploads the same way, so that a scanner whose descriptor has no efn() in its score section can evaluate
 * structures.  Loading changes no scan (a scan's energy kernel runs for the descriptor's call sites only); tables
 * loaded again replace those that are there; the call is refused while a scan is in flight.
 * Structure s is the bases [ off[ s ], off[ s + 1 ] ) of d_base and d_pair.  d_base holds letters, as
 * rma_hit_structures' base; letters: 256 bytes, byte -> letter, or NULL for the readers' letters; a c g t/u in either
 * case are codes 0..3, every other letter is ambiguous.  d_pair[ ( off[ s ] + i ) * pair_stride ] is the index inside
 * the structure of the base that i pairs with, or -1 -- rma_hit_structures' mate: with pair_stride 3, column 0 of a
 * mate tensor is read in place.  Pairs are taken as given, as the drivers take a .ct file: no pair set filters them.
 * d_efn / d_efn2 (either may be NULL) receive the energies in 1/100 kcal/mol, as the efn words of a hit record:
 * RMA_EFN_INFINITY / RMA_EFN2_INFINITY where the cores say so, for a structure of no bases, for a structure with
 * crossing pairs and for one with a pair (i, i+1), which closes no loop.  Asking for an energy whose tables the
 * scanner does not have is an error before anything is launched.
 * Pointers are checked as rma_hit_structures checks its outputs.  Every structure is checked on the device, in one
 * kernel with one wait, before any energy is computed: off[ 0 ] == 0, off ascending, off[ n ] == total; at most 8191
 * bases (RMA_EFN_LOGINC - 1: no loop size is ever clamped); every partner -1 or inside its structure, not the base
 * itself, and returned by its partner; at most 50 helices, a pair (i, j) opening a new helix unless (i-1, j+1) is a
 * pair.  A bad structure fails the call, naming the lowest bad structure's index and the reason, and nothing is
 * written.  n == 0 does nothing.  The kernels are queued on `stream` (the caller's hipStream_t, NULL = the default
 * stream) behind what is queued there now and ahead of what is queued there next; the call returns without waiting
 * for the energy kernel.  Scratch (512 bytes + 4 per structure) is the scanner's, made on the first call and grown.
 * Option "struct_wgs" (rma_scanner_set_option) sets the number of workgroups of the kernels, 0 for the default. */
int	rma_scanner_load_energy_tables( rma_scanner_t *sc, const char *dir, int which /* 1 efn, 2 efn2, 3 both */,
		char *err, size_t errlen );
int	rma_structure_energies( rma_scanner_t *sc, const int64_t *d_off /* n+1 */, const uint8_t *d_base /* total */,
		const int32_t *d_pair /* total * pair_stride */, int32_t pair_stride, int64_t n, int64_t total,
		const uint8_t *letters /* 256, host, or NULL */,
		int32_t *d_efn /* n or NULL */, int32_t *d_efn2 /* n or NULL */, void *stream, char *err, size_t errlen );

/* ---- the score section on the device: which records are hits, and their SCORE (csrc/rm_score_core.h has the rule,
 * one function shared by the host and the kernel; csrc/rm_score_image.h the image it runs and its limits).
 * rma_score_open() compiles a private copy of d (d itself is not touched), runs BEGIN on it and translates MAIN into
 * an image.  It refuses with words, and makes no image, where records cannot be judged one by one on the device:
 * MAIN is not independent from hit to hit (ScoreVM::hit_independent's reason: HOLD / RELEASE, a variable carried from
 * one hit to the next); MAIN calls sprintf(), bits() or mismatches( string, pattern ), uses =~ or !~, or reads NAME;
 * the descriptor is loose (rma_program_loose() > 0: its records are not yet the reference's candidates); the image
 * is larger than the limits of rm_score_image.h, or would leave no room in LDS for one wave.  A descriptor without a
 * MAIN program opens: every record is accepted, with SCORE as BEGIN left it (kind 0 unless BEGIN assigns it). */
int	rma_score_open( const rma_descr_t *d, rma_score_t **out, char *err, size_t errlen );
void	rma_score_close( rma_score_t *sp );
/* What an image and its kernel take (profiles/score_device.py): info[ 0 ] bytes of the image, [ 1 ] instructions,
 * [ 2 ] variables, [ 3 ] slots of the operand stack, [ 4 ] bytes of LDS a wave's stack and variables take, [ 5 ] waves of
 * a workgroup, [ 6 ] bytes of dynamic LDS of a workgroup; from the runtime, -1 each where no device answers: [ 7 ] bytes
 * of private memory a lane of rma_score_kernel has, [ 8 ] its static LDS, [ 9 ] its registers -- of the instance that
 * would run the image: rma_score_text_kernel with RMA_SCORE_TEXT, rma_score_match_kernel / rma_score_match_text_kernel
 * for a program opened with RMA_SCORE_MATCH that has a pattern, whose [ 4 ] and [ 6 ] then hold the matcher's stack too. */
void	rma_score_info( const rma_score_t *sp, int32_t info[ 10 ] );
/* rma_score_hits(): MAIN on each of the n_hits records at d_hits, one record per lane.  d_accept[ h ] = 1 where record h
 * is a hit (ACCEPT, or MAIN's end is never reached without one), 0 where MAIN rejects it; d_score[ h ] the SCORE the
 * printer would read, an int as its exact double, d_kind[ h ] 0 for none, 1 for an int, 2 for a float (either may be
 * NULL); a rejected record has score 0.0 of kind 0.  Doubles are the host VM's bit for bit.
 * Arguments as rma_hit_structures takes them: any rows of a scan's records in any order; db made by
 * rma_db_create_device*() (its text is read in place, through `letters` -- 256 bytes, none 0, or NULL -- as
 * rma_replay_device() reads it); the pointers checked against their allocations on the scanner's device; the
 * program of sp must be the scanner's, byte for byte.  Every record is checked on the device by rma_replay_device()'s
 * rule before anything it points to is read; a bad record fails the call, naming its index.  A record on which MAIN
 * stops fails the call too: err names the lowest such record, file and line of the instruction and the reason in the
 * host VM's words -- type mismatch, undefined variable, bad pos / len, integer division by zero, '$' outside a
 * reference, element stack overflow ... -- or one of the three stops the host VM has not: string + string (needs a
 * buffer), a string in SCORE at ACCEPT, and more instructions for one record than option "score_budget"
 * (rma_scanner_set_option; 2^20 unless set) allows, so that no score program can hold the device.
 * After a failed call the outputs hold what they held before: results go to scratch of the scanner's (10 bytes a
 * record, made on the first call and grown) and are copied once the check has passed.  The work runs on a stream of
 * the scanner's own, behind what is queued on `stream` (the caller's hipStream_t, NULL = the default stream) and
 * ahead of what is queued there next; the call waits once.  n_hits == 0 does nothing. */
int	rma_score_hits( rma_scanner_t *sc, const rma_score_t *sp, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
		const uint8_t *letters /* 256 or NULL */, uint8_t *d_accept /* n */, double *d_score /* n or NULL */,
		int8_t *d_kind /* n or NULL: 0 none, 1 int, 2 float */, void *stream, char *err, size_t errlen );

/* ---- loose seq= expressions on the device: which records are rnamotif's candidates (csrc/rm_seqcheck.h has the rule,
 * one function shared by the host and the kernel, and the image it runs with its limits).  The records of a descriptor
 * with rma_program_loose() > 0 are a superset of the reference's candidates: the scan tests a necessary condition for a
 * seq= with a \( \) group and a back reference, with \< or \>, or -- iupac = 0 -- with a letter that is not acgt.
 * rma_seqcheck_hits() applies the expressions themselves to the element text of each record, as rma_replay_*() does on
 * the host before it counts a candidate (step(), or mm_step() where the element has a mismatch limit).
 * rma_seqcheck_open() flattens the loose expressions of d into an image; a descriptor that is not loose opens with zero
 * expressions, so that one pipeline serves every descriptor.  Refused with words: more than 20 loose elements, more
 * than 255 ops in one expression, an image that leaves no room in 64 KB of LDS for the stack of one wave. */
typedef struct rma_seqcheck	rma_seqcheck_t;
int	rma_seqcheck_open( const rma_descr_t *d, rma_seqcheck_t **out, char *err, size_t errlen );
void	rma_seqcheck_close( rma_seqcheck_t *sq );
/* What an image and its kernel take (profiles/seq_check.py): info[ 0 ] expressions, [ 1 ] ops of all of them, [ 2 ] frames
 * of the matcher's stack (the most repeating ops of one expression), [ 3 ] bytes of the image, [ 4 ] waves of a
 * workgroup, [ 5 ] bytes of dynamic LDS of a workgroup; from the runtime, -1 each where no device answers: [ 6 ] bytes of
 * private memory a lane of rma_seqcheck_kernel has, [ 7 ] its registers. */
void	rma_seqcheck_info( const rma_seqcheck_t *sq, int32_t info[ 8 ] );
/* rma_seqcheck_hits(): d_keep[ h ] = 1 where record h passes every loose expression -- it is a candidate of the
 * reference's -- and 0 where it is dropped at the first that fails, in the order of the elements.  d_fixed (or NULL):
 * the records again, n_hits * stride words, with word RMA_HIT_HDR + 4 * e + 3 of a kept record replaced by mm_step()'s
 * mismatch count for every loose element e with a mismatch limit, as the replay fixes it before the score section
 * reads it; a dropped record's row is the input row.  d_hits[ d_keep ] of the fixed rows are what rma_score_hits of a
 * program opened by rma_score_open_checked() takes.  d_fixed may not overlap d_hits.
 * Arguments as rma_score_hits takes them: any rows of a scan's records in any order; db made by
 * rma_db_create_device*() (its text is read in place, through `letters` -- 256 bytes, none 0, or NULL); the pointers
 * checked against their allocations on the scanner's device; the program of sq must be the scanner's, byte for byte.
 * Every record is checked on the device by rma_replay_device()'s rule before anything it points to is read; a bad
 * record fails the call, naming its index.  budget: the ops one record may visit, 0 for 2^20 -- backtracking over an
 * expression like .*\(..\).*\1 grows fast with the element's length, and no expression may hold the device; a record
 * that needs more fails the call: err names the lowest such record, its element and the budget.  An element's text ends
 * where the element ends: nothing behind it is read.
 * After a failed call the outputs hold what they held before: results go to scratch of the scanner's and are copied
 * once the check has passed.  The work runs on a stream of the scanner's own, behind what is queued on `stream` (the
 * caller's hipStream_t, NULL = the default stream) and ahead of what is queued there next; the call waits once.
 * n_hits == 0 does nothing. */
int	rma_seqcheck_hits( rma_scanner_t *sc, const rma_seqcheck_t *sq, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
		const uint8_t *letters /* 256 or NULL */, int32_t budget /* 0: 2^20 */,
		uint8_t *d_keep /* n_hits */, int32_t *d_fixed /* n_hits * stride, or NULL */, void *stream, char *err, size_t errlen );
/* rma_score_open() without its refusal of a loose descriptor; every other refusal and every limit stays.  The caller
 * promises that the records it will pass to rma_score_hits() passed rma_seqcheck_hits() (d_keep 1) and are its fixed
 * rows: on any other record of a loose descriptor MAIN judges what the reference never scored. */
int	rma_score_open_checked( const rma_descr_t *d, rma_score_t **out, char *err, size_t errlen );

/* ---- the score section on the device with text: sprintf(), bits(), string + and a string in SCORE.
 * rma_score_open_flags(): flags 0 is rma_score_open(), RMA_SCORE_CHECKED rma_score_open_checked().  With RMA_SCORE_TEXT
 * the refusals of sprintf() and bits() fall -- every other refusal and limit stays -- and a record has a heap of option
 * "score_heap" bytes (rma_scanner_set_option; 256 unless set) in which string + and sprintf() make their strings:
 * a string that does not fit stops the record.  sprintf() writes %d %i %u %o %x %X of an int, %s of a string, %f of a
 * float, %n and %% with the flags - + blank 0 #, a width and a precision, the bytes of the host's snprintf (%f: every
 * finite double below 2^63 in magnitude, a precision up to 18).  What the host VM only notes as an error -- a wrong
 * argument type, no such argument, an unsupported conversion -- stops the record, as do '*', '$' and length modifiers,
 * %e %E %g %G (refused when the program is opened where the format is a constant), a larger precision and a double %f
 * cannot write.  bits() reads the host's own logarithms from a table made when the program is opened, for windows of up
 * to L bases -- the sum of the elements' greatest lengths, at most 1024; a longer window stops the record.
 * With RMA_SCORE_MATCH the refusals of =~, !~ and mismatches( string, pattern ) fall, in any combination with the other
 * two flags: the pattern of each is compiled when the program is opened (compile() of the reference's regexp.c, as
 * rma_seqcheck_open() compiles a loose seq=) and applied to each record's string by the reference's step() / advance() /
 * mm_step(), the rule of csrc/rm_seqcheck.h, whose stack lives in LDS beside the program's.  Refused when opened, each
 * with file and line: a pattern that is not one string constant (a variable, an element reference, sprintf(), string +:
 * it would have to be compiled for every record), a constant compile() rejects (the words name it and the regerr
 * code; "" alone opens, and matches nothing, as on the host), more than 32 patterns, more than 255 ops in one, an image
 * that with the matcher's stack leaves no room for one wave in 64 KB of LDS.  NAME, HOLD / RELEASE and a variable
 * carried from hit to hit stay refused.  =~ on something that is no string stops the record with the host VM's word,
 * "typemismatch."; every op the matcher visits counts against option "score_budget" with the instructions, so that a
 * backtracking pattern over a long made string holds the device no longer than a loop may.  Without the flag every
 * refusal keeps its words, and a program opened with it that has no such pattern runs the kernels it ran. */
#define RMA_SCORE_CHECKED 1u   /* as rma_score_open_checked() */
#define RMA_SCORE_TEXT    2u   /* sprintf(), bits(), string +, a string in SCORE */
/* (8, not 4: bit 4 stays refused, "flags other than ...", as callers and tests of rma_score_open_flags() know it) */
#define RMA_SCORE_MATCH   8u   /* =~, !~ and mismatches( string, pattern ) with a constant pattern */
int	rma_score_open_flags( const rma_descr_t *d, unsigned flags, rma_score_t **out, char *err, size_t errlen );
/* rma_score_hits() with the score column as bytes.  Row h of d_text (text_stride bytes a row) is the field
 * HitPrinter::print writes behind the one blank after the name: %8d of an int SCORE, %8.3lf of a float or of none, %8s
 * of a string; d_text_len[ h ] is its length (at least 8; 0 for a rejected record), bytes behind it are not written.
 * d_kind[ h ] is 3 for a string SCORE, whose d_score[ h ] is 0.0.  A field longer than text_stride stops the record, as
 * does a float SCORE %8.3lf cannot write alike on host and device (not finite, 2^63 or more).  The program may be
 * opened with or without RMA_SCORE_TEXT, as rma_score_hits() takes both (and stops on a string SCORE).
 * Everything else as rma_score_hits(): the checks, chunks of 2^17 records, results in scratch of the scanner's until
 * the check has passed, a failed call writes nothing, one wait, the order on the caller's stream. */
int	rma_score_hits_text( rma_scanner_t *sc, const rma_score_t *sp, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,
		const uint8_t *letters, uint8_t *d_accept, double *d_score /* or NULL */, int8_t *d_kind /* or NULL */,
		uint8_t *d_text /* n_hits * text_stride */, int32_t text_stride, int32_t *d_text_len /* n_hits */,
		void *stream, char *err, size_t errlen );

/* ---- hit records as rnamotif prints them, on the device: for each of the n_hits records at d_hits the two lines
 * HitPrinter::print puts on stdout -- ">sid sdef" and the hit line: %-12s of sid, the score column, " %d %7d %4d" of
 * strand, offset and length, one field per printed element -- as bytes in device memory (csrc/rm_hitprint.h has the
 * rule, shared by the host and the kernels).  The score column of record h is the d_text_len[ h ] bytes of row h of
 * d_text_bytes, as rma_score_hits_text() delivers them; a record whose d_accept[ h ] is 0 has no bytes (d_accept
 * NULL: every record is printed).  Record h is bytes [ d_off[ h ], d_off[ h + 1 ] ) of d_out, in the order given:
 * d_out copied to the host and written behind rma_print_header()'s bytes is rnamotif's output for these records.
 * The names of the entries come from a table on the device.  rma_names_create() makes it for a database made by
 * rma_db_create_device() or rma_db_create_device_fasta(): n (the database's number of entries) sids and sdefs, each a
 * C string or, with sid_len / sdef_len given, that many bytes without a NUL; sids NULL or sids[ e ] NULL: the entry's
 * number in decimal -- for a database made from FASTA text its own rma_db_entry_name() -- and sdefs likewise: "", or
 * the database's own.  A sid of 2048 bytes or more is refused: the printer would cut it.  The table is uploaded once,
 * on the device's upload stream behind the database, and the call does not wait; rma_names_destroy() waits for the
 * kernels that read it.
 * Arguments as rma_hit_structures takes them: any rows in any order, the checks (a bad record fails the call, naming
 * its index, as does a d_text_len[ h ] outside [0, text_width]; nothing is written then), chunks of 2^17 records,
 * pointers checked alike.  rma_hit_print_size() returns the bytes of all records in *total and synchronises once.
 * rma_hit_print() checks and counts again, refuses a total that is not what it finds, then queues the kernel that
 * fills d_out and d_off and returns without waiting for it: it runs behind what is queued on `stream` now and ahead of
 * what is queued there next.  Names made for another database are refused.  rma_print_header() writes the three "#RM"
 * lines HitPrinter::header prints in front of the first hit into buf (NUL-terminated, cut at buflen - 1 bytes) and
 * returns their length, -1 when it cannot. */
typedef struct rma_names	rma_names_t;
int	rma_names_create( rma_scanner_t *sc, const rma_db_t *db, const char *const *sids, const int64_t *sid_len /* or NULL */,
		const char *const *sdefs, const int64_t *sdef_len /* or NULL */, int32_t n, rma_names_t **out,
		char *err, size_t errlen );
void	rma_names_destroy( rma_names_t *names );
int	rma_hit_print_size( rma_scanner_t *sc, const rma_db_t *db, const rma_names_t *names, const int32_t *d_hits, int64_t n_hits,
		const uint8_t *d_accept /* n_hits or NULL: all */, const int32_t *d_text_len /* n_hits */,
		int64_t *total, void *stream, char *err, size_t errlen );
int	rma_hit_print( rma_scanner_t *sc, const rma_db_t *db, const rma_names_t *names, const int32_t *d_hits, int64_t n_hits,
		const uint8_t *letters /* 256 or NULL */, const uint8_t *d_accept, const uint8_t *d_text_bytes, int32_t text_width,
		const int32_t *d_text_len, int64_t total, uint8_t *d_out /* total */, int64_t *d_off /* n_hits + 1 */,
		void *stream, char *err, size_t errlen );
int	rma_print_header( const rma_descr_t *d, char *buf, size_t buflen );

/* ---- hit records as rmfmt lists them, on the device: what `rmfmt`, `rmfmt -l` (RMA_LIST_LOCUS) or `rmfmt -la`
 * (RMA_LIST_ACC) makes of rma_hit_print()'s bytes for the same arguments -- the printed records sorted (best score
 * first where the score column is one number, else by name and position), every field padded to its widest instance,
 * elements of more than 20 letters abbreviated -- as n_lines lines of line_len bytes each in device memory, with the
 * permutation: line r is record d_perm[ r ] (csrc/rm_hitlist.h has the rule, shared by the host and the kernels).
 * The lines written behind rma_print_header()'s bytes are rmfmt's output.  smax <= 0 means rmfmt's 30 000 000: a
 * listing whose raw temp file would be larger keeps the input order (*mode 0; 1: by score; 2: by name).
 * Arguments, checks, chunks and names as rma_hit_print takes them.  Refused as well, the least record named and
 * nothing written: printed records that do not all have the same number (at least one) of score fields -- rmfmt's
 * result for them depends on the line it read last, which is not restated --, a newline in a score column, a line of
 * more than 200 fields, a hit line of 50 000 bytes or more; an entry whose name is empty, trims to nothing or holds a
 * blank, a tab or a newline; letters that map a byte to one of these three.
 * rma_hit_list_shape() gives the lines, their length, the widths (host: name, score block, comp, offset, len, then one
 * per column of rma_hit_alignment_shape(); room for 5 + RMA_MAX_ELEMS + 2) and the mode, and synchronises once.
 * rma_hit_list() checks and measures again, refuses a shape that is not what it finds, then queues the sort and the
 * fill and returns without waiting for them, ordered with `stream` as rma_hit_print() is. */
enum { RMA_LIST_WHOLE = 0, RMA_LIST_LOCUS = 1, RMA_LIST_ACC = 2 };
int	rma_hit_list_shape( rma_scanner_t *sc, const rma_db_t *db, const rma_names_t *names, const int32_t *d_hits, int64_t n_hits,
		const uint8_t *d_accept /* n_hits or NULL: all */, const uint8_t *d_text_bytes, int32_t text_width,
		const int32_t *d_text_len /* n_hits */, int32_t name_mode, int64_t smax, int64_t *n_lines, int64_t *line_len,
		int32_t *widths, int32_t *mode, void *stream, char *err, size_t errlen );
int	rma_hit_list( rma_scanner_t *sc, const rma_db_t *db, const rma_names_t *names, const int32_t *d_hits, int64_t n_hits,
		const uint8_t *d_accept, const uint8_t *d_text_bytes, int32_t text_width, const int32_t *d_text_len,
		int32_t name_mode, int64_t smax, const uint8_t *letters /* 256 or NULL */, int64_t n_lines, int64_t line_len,
		uint8_t *d_lines /* n_lines * line_len */, int64_t *d_perm /* n_lines */, void *stream, char *err, size_t errlen );

/* ---- hit records as rm2ct writes them, on the device: what `rm2ct` (RMA_CT_RNAMOTIF) or `rm2ct -t rnaviz`
 * (RMA_CT_RNAVIZ) makes of rma_hit_print()'s bytes for the same arguments -- per printed record a header line and one
 * line per base with its number, its neighbours, its partner and its place in the entry -- as one run of bytes in device
 * memory (csrc/rm_hitct.h has the rule, shared by the host and the kernels).  rm2ct pairs by the words of the
 * "#RM descr" line, so the call takes them: descr_words is what rma_descr_names() gives for the scanner's descriptor.
 * The partner is the tool's: counted from 0 in p5/p3, -1 for a context's base.  rnaviz prints the number the tool reads
 * behind the name with atof(), as a float.
 * Arguments, checks, chunks, names and the two calls as rma_hit_print takes them: rma_hit_ct_size() returns the bytes of
 * all records in *total and synchronises once; rma_hit_ct() checks and counts again, refuses another total, queues the
 * fill and returns without waiting for it, ordered with `stream` as rma_hit_print() is.  Refused before a record is
 * looked at: a descriptor with a triple or quad helix, in the tool's words; a type that is neither; an entry whose name
 * is empty or holds a blank, a tab, a newline or another space; letters that map a byte to something that is no ASCII
 * letter (the tool counts bases with isalpha).  Refused naming the least record, nothing written: a bad record, a
 * d_text_len[ h ] outside [0, text_width], a newline in a score column, a hit line of 50 000 bytes or more (the tool's
 * line buffer) and, for rnaviz, a text behind the name that is an inf, nan, 0x or exponent form of strtod's, has more
 * than 19 digits from its first non-zero digit to its last or behind the point. */
enum { RMA_CT_RNAMOTIF = 0, RMA_CT_RNAVIZ = 1 };
int	rma_hit_ct_size( rma_scanner_t *sc, const rma_db_t *db, const rma_names_t *names, const int32_t *d_hits, int64_t n_hits,
		const uint8_t *d_accept /* n_hits or NULL: all */, const uint8_t *d_text_bytes, int32_t text_width,
		const int32_t *d_text_len /* n_hits */, int32_t type, const char *descr_words, const uint8_t *letters /* 256 or NULL */,
		int64_t *total, void *stream, char *err, size_t errlen );
int	rma_hit_ct( rma_scanner_t *sc, const rma_db_t *db, const rma_names_t *names, const int32_t *d_hits, int64_t n_hits,
		const uint8_t *d_accept, const uint8_t *d_text_bytes, int32_t text_width, const int32_t *d_text_len, int32_t type,
		const char *descr_words, const uint8_t *letters, int64_t total, uint8_t *d_out /* total */, int64_t *d_off /* n_hits + 1 */,
		void *stream, char *err, size_t errlen );

#ifdef __cplusplus
}
#endif
#endif
