/* ref_find_motif_drv.c -- TEST INFRASTRUCTURE.
 *
 * A driver of this repository's own around the reference's matcher, compiled together with
 * /root/reference/src/find_motif.c, regexp.c, mm_regexp.c and log.c where they lie (oracle/Makefile,
 * target ref; never copied, never committed as a binary).  The reference's parser needs yacc/lex
 * output and is not built; the matcher needs none of it: it reads the compiled descriptor from
 * process globals (find_motif.c:17-43), and rma_program_t (include/rnamotif_amd_program.h) is a
 * flat copy of exactly those.  This driver goes back from the blob to the globals, calls
 * RM_fm_init() once and RM_find_motif() per entry and strand the way main() does
 * (rnamot.c:151-185), and defines RM_score() itself: the reference calls it at the point where a
 * candidate has passed chk_motif, set_context and chk_sites (find_motif.c:364-386), so the
 * driver sees the reference's candidates, their fields and their order, one line per call:
 *
 *   entry strand  { s_matchoff s_matchlen s_n_mispairs s_n_mismatches } per element
 *                 lctx off len  rctx off len          (0 0 where there is none)
 *
 *   find_motif_drv [-z] program-file sequence-file
 *
 * program-file: the bytes of an rma_program_t, then per element that has a seq= the string as the
 * parser leaves it in s_seq (after RM_str2seq's IUPAC expansion): int32 element (-1 lctx, -2 rctx),
 * int32 length, the bytes; closed by element -3 (tests/hostsim/program_dump.cpp writes it).
 * sequence-file: one entry per line, an empty line is an empty entry.
 *
 * What the driver decides, and why:
 *  - rm_o_stp = NULL.  The -O best-literal skip (adjust_szero, find_motif.c:209) is an optimisation
 *    of the reference's, and the blob does not carry s_bestpat: every start position is visited.
 *  - RM_score() returns SA_REJECT, so print_match() stays out of it.  The rv values of the find_*
 *    functions are only OR-ed upwards (find_motif.c:193,279,458,524,634,842,895,967); no search
 *    decision reads them.
 *  - fm_window[] is never initialised by the reference (find_motif.c:129).  find_motif.c is
 *    compiled with -Dmalloc=drv_malloc: the allocator below fills what it hands out, and a margin
 *    on both sides, with the bytes of UNDEF (-1), or with zeros under -z.
 *  - The strict-helix checks index descr[] with what fm_window[] holds, UNDEF included
 *    (find_motif.c:1482-1483 and the like): rm_descr[ -1 ].  rm_descr is therefore the second
 *    element of a zeroed array here, so that the element before it has s_type 0, which is no
 *    SYM_* -- what a neighbour in .bss gives the reference.
 *  - s_n_mismatches / s_n_mispairs start as SE_init leaves them (UNDEF, compile.c:570-571) and are
 *    carried from one strand and entry to the next, as in the reference's process.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

#include "rmdefs.h"
#include "rnamot.h"
#include "y.tab.h"
#include "rnamotif_amd_program.h"

extern	int	circf;
extern	void	compile( char *, register char *, char *, int );

#define	DESCR_SIZE	100			/* compile.c:49 */
STREL_T	drv_descr_store[ DESCR_SIZE + 1 ];	/* rm_descr = &drv_descr_store[ 1 ], see below */
extern	STREL_T	rm_descr[];
int	rm_n_descr;
int	rm_dminlen, rm_dmaxlen;
STREL_T	*rm_o_stp = NULL;
char	*rm_o_expbuf = NULL;
STREL_T	*rm_lctx = NULL, *rm_rctx = NULL;
int	rm_lctx_explicit, rm_rctx_explicit;
SITE_T	*rm_sites = NULL;
int	rm_b2bc[ 256 ];
SEARCH_T	**rm_searches;
int	rm_n_searches;
ARGS_T	*rm_args;
int	rm_error;
char	*rm_wdfname = "program";
static	VALUE_T	v_n, v_s, v_c, v_p, v_l;
VALUE_T	*rm_nval = &v_n, *rm_sval = &v_s, *rm_cval = &v_c, *rm_pval = &v_p, *rm_lval = &v_l;

/* rm_descr[ -1 ] must be memory of ours: the symbol is set one element into the array */
static void __attribute__(( used )) drv_place_descr( void )
{
	__asm__( ".globl rm_descr\n\t.set rm_descr, drv_descr_store + %c0" : : "i"( sizeof( STREL_T ) ) );
}

static	int	fill_byte = 0xff;
#define	MARGIN	65536
void	*drv_malloc( size_t n )
{
	char	*p = ( char * )malloc( n + 2 * MARGIN );

	if( p == NULL )
		return( NULL );
	memset( p, fill_byte, n + 2 * MARGIN );
	return( p + MARGIN );
}

static	ARGS_T	args;
static	IDENT_T	id_windowsize;
static	STREL_T	lctx, rctx;
static	PAIRSET_T	pairsets[ RMA_MAX_PAIRSETS ];
static	int	cur_entry;

IDENT_T	*RM_find_id( char name[] )
{
	return( !strcmp( name, "windowsize" ) ? &id_windowsize : NULL );
}

void	RM_strel_name( STREL_T *stp, char name[] )	/* (print_match only) */
{
	strcpy( name, "?" );
}

int	RM_score( int comp, int slen, char sbuf[], IDENT_T **h_idp )
{
	int	d;
	STREL_T	*stp;

	printf( "%d %d", cur_entry, comp );
	for( stp = rm_descr, d = 0; d < rm_n_descr; d++, stp++ )
		printf( " %d %d %d %d", stp->s_matchoff, stp->s_matchlen, stp->s_n_mispairs, stp->s_n_mismatches );
	if( rm_lctx != NULL )
		printf( " %d %d", rm_lctx->s_matchoff, rm_lctx->s_matchlen );
	else
		printf( " 0 0" );
	if( rm_rctx != NULL )
		printf( " %d %d", rm_rctx->s_matchoff, rm_rctx->s_matchlen );
	else
		printf( " 0 0" );
	putchar( '\n' );
	if( h_idp != NULL )
		*h_idp = NULL;
	return( SA_REJECT );
}

static	int	sym_of( int type )
{
	static const int	sym[] = { SYM_CTX, SYM_SS, SYM_H5, SYM_H3, SYM_P5, SYM_P3,
		SYM_T1, SYM_T2, SYM_T3, SYM_Q1, SYM_Q2, SYM_Q3, SYM_Q4, SYM_SE };

	return( sym[ type ] );
}

static	STREL_T	*elem_ptr( int i )
{
	return( i < 0 ? NULL : &rm_descr[ i ] );
}

static	PAIRSET_T	*pairset_of( const rma_program_t *p, int ps )
{
	const rma_pairset_t	*r;
	PAIRSET_T	*o;
	int	*m, i;

	if( ps < 0 )
		return( NULL );
	o = &pairsets[ ps ];
	if( o->ps_mat[ 0 ] != NULL )
		return( o );
	r = &p->pairsets[ ps ];
	m = ( int * )calloc( 25, sizeof( int ) );		/* BP_MAT_T */
	for( i = 0; i < 25; i++ )
		m[ i ] = ( r->mat2 >> i ) & 1;
	o->ps_mat[ 0 ] = m;
	if( r->n_bases == 3 ){
		m = ( int * )calloc( 125, sizeof( int ) );	/* BT_MAT_T */
		for( i = 0; i < 125; i++ )
			m[ i ] = ( r->mat3[ i >> 5 ] >> ( i & 31 ) ) & 1;
		o->ps_mat[ 1 ] = m;
	}else if( r->n_bases == 4 ){
		m = ( int * )calloc( 625, sizeof( int ) );	/* BQ_MAT_T */
		for( i = 0; i < 625; i++ )
			m[ i ] = ( r->mat4[ i >> 5 ] >> ( i & 31 ) ) & 1;
		o->ps_mat[ 1 ] = m;
	}
	return( o );
}

static	void	cvt( const rma_program_t *p, const rma_elem_t *e, STREL_T *stp )
{
	int	i;

	memset( stp, 0, sizeof( *stp ) );
	stp->s_type = sym_of( e->type );
	stp->s_attr[ SA_PROPER ] = e->proper;
	stp->s_attr[ SA_ENDS ] = e->ends;
	stp->s_attr[ SA_STRICT ] = e->strict;
	stp->s_index = e->index;
	stp->s_searchno = e->searchno;
	stp->s_matchoff = stp->s_matchlen = UNDEF;
	stp->s_n_mismatches = stp->s_n_mispairs = UNDEF;
	stp->s_next = elem_ptr( e->next );
	stp->s_prev = elem_ptr( e->prev );
	stp->s_inner = elem_ptr( e->inner );
	stp->s_outer = elem_ptr( e->outer );
	stp->s_n_mates = e->n_mates;
	if( e->n_mates > 0 ){
		stp->s_mates = ( STREL_T ** )calloc( e->n_mates, sizeof( STREL_T * ) );
		for( i = 0; i < e->n_mates; i++ )
			stp->s_mates[ i ] = elem_ptr( e->mates[ i ] );
	}
	stp->s_n_scopes = e->n_scopes;
	if( e->n_scopes > 0 ){
		stp->s_scopes = ( STREL_T ** )calloc( e->n_scopes, sizeof( STREL_T * ) );
		for( i = 0; i < e->n_scopes; i++ )
			stp->s_scopes[ i ] = elem_ptr( e->scopes[ i ] );
	}
	stp->s_scope = e->scope;
	stp->s_minlen = e->minlen;
	stp->s_maxlen = e->maxlen;
	stp->s_minglen = e->minglen;
	stp->s_maxglen = e->maxglen;
	stp->s_minilen = e->minilen;
	stp->s_maxilen = e->maxilen;
	stp->s_mismatch = e->mismatch;
	stp->s_matchfrac = 1.0;
	stp->s_mispair = e->mispair;
	stp->s_pairfrac = e->pairfrac;
	stp->s_pairset = pairset_of( p, e->pairset );
}

static	void	set_seq( STREL_T *stp, char *seq )	/* compile.c:1542-1555 */
{
	size_t	size = RE_BPC * strlen( seq );

	stp->s_seq = seq;
	stp->s_expbuf = ( char * )calloc( size + 1, 1 );
	stp->s_e_expbuf = &stp->s_expbuf[ size ];
	compile( stp->s_seq, stp->s_expbuf, stp->s_e_expbuf, '\0' );
}

static	void	die( const char *msg, const char *what )
{
	fprintf( stderr, "find_motif_drv: %s %s\n", msg, what );
	exit( 2 );
}

static	void	load_program( const char *fname )
{
	FILE	*fp = fopen( fname, "rb" );
	rma_program_t	*p = ( rma_program_t * )malloc( sizeof( rma_program_t ) );
	int	i, s;
	int32_t	hdr[ 2 ];
	SITE_T	*sip, **tail;

	if( fp == NULL || fread( p, sizeof( *p ), 1, fp ) != 1 )
		die( "can't read program", fname );
	if( p->magic != RMA_MAGIC || p->size != sizeof( *p ) )
		die( "not a program of this build:", fname );

	rm_n_descr = p->n_elems;
	for( i = 0; i < p->n_elems; i++ )
		cvt( p, &p->elems[ i ], &rm_descr[ i ] );
	if( p->has_lctx ){
		cvt( p, &p->lctx, &lctx );
		rm_lctx = &lctx;
	}
	if( p->has_rctx ){
		cvt( p, &p->rctx, &rctx );
		rm_rctx = &rctx;
	}
	rm_dminlen = p->dminlen;
	rm_dmaxlen = p->dmaxlen;

	/* rm_searches[] and its links, set_search_order_links compile.c:3290 */
	rm_n_searches = p->n_searches;
	rm_searches = ( SEARCH_T ** )calloc( p->n_elems + 1, sizeof( SEARCH_T * ) );
	for( s = 0; s < p->n_searches; s++ ){
		rm_searches[ s ] = ( SEARCH_T * )calloc( 1, sizeof( SEARCH_T ) );
		rm_searches[ s ]->s_descr = &rm_descr[ p->searches[ s ] ];
		rm_searches[ s ]->s_zero = rm_searches[ s ]->s_dollar = UNDEF;
	}
	for( s = 0; s < p->n_searches - 1; s++ )
		rm_searches[ s ]->s_forward = rm_searches[ s + 1 ]->s_descr;
	for( s = 1; s < p->n_searches; s++ ){
		STREL_T	*stp = rm_searches[ s ]->s_descr, *stp1;
		if( stp->s_prev != NULL )
			rm_searches[ s ]->s_backup = stp->s_prev;
		else if( ( stp1 = stp->s_outer ) == NULL )
			rm_searches[ s ]->s_backup = NULL;
		else
			rm_searches[ s ]->s_backup = stp1->s_attr[ SA_PROPER ] ? stp1 : stp1->s_scopes[ 0 ];
	}

	for( tail = &rm_sites, s = 0; s < p->n_sites; s++ ){
		const rma_site_t	*rs = &p->sites[ s ];
		sip = ( SITE_T * )calloc( 1, sizeof( SITE_T ) );
		sip->s_n_pos = rs->n_pos;
		sip->s_pos = ( POS_T * )calloc( rs->n_pos, sizeof( POS_T ) );
		for( i = 0; i < rs->n_pos; i++ ){
			sip->s_pos[ i ].p_descr = &rm_descr[ rs->pos[ i ].elem ];
			sip->s_pos[ i ].p_addr.a_l2r = rs->pos[ i ].l2r;
			sip->s_pos[ i ].p_addr.a_offset = rs->pos[ i ].offset;
		}
		sip->s_pairset = pairset_of( p, rs->pairset );
		*tail = sip;
		tail = &sip->s_next;
	}

	/* letter -> base code as RM_init sets it up (compile.c:180-187): acgt and u as t, either case; all else N */
	{
		static const char	letters[] = "aAcCgGtTuU";
		static const int	codes[] = { BCODE_A, BCODE_C, BCODE_G, BCODE_T, BCODE_T };
		for( i = 0; i < 256; i++ )
			rm_b2bc[ i ] = BCODE_N;
		for( i = 0; letters[ i ] != '\0'; i++ )
			rm_b2bc[ ( unsigned char )letters[ i ] ] = codes[ i / 2 ];
	}

	args.a_strict_helices = p->strict_helices;
	rm_args = &args;
	id_windowsize.i_name = "windowsize";
	id_windowsize.i_type = T_INT;
	id_windowsize.i_val.v_type = T_INT;
	id_windowsize.i_val.v_value.v_ival = p->windowsize;
	args.a_copt = p->chk_both_strs;			/* (kept here for main(); the matcher does not read it) */

	for( ; ; ){
		char	*seq;
		STREL_T	*stp;
		if( fread( hdr, sizeof( hdr ), 1, fp ) != 1 )
			die( "seq= strings cut short in", fname );
		if( hdr[ 0 ] == -3 )
			break;
		if( hdr[ 0 ] < -2 || hdr[ 0 ] >= p->n_elems || hdr[ 1 ] < 0 )
			die( "bad seq= record in", fname );
		seq = ( char * )calloc( ( size_t )hdr[ 1 ] + 1, 1 );
		if( hdr[ 1 ] > 0 && fread( seq, ( size_t )hdr[ 1 ], 1, fp ) != 1 )
			die( "seq= strings cut short in", fname );
		stp = hdr[ 0 ] == -1 ? rm_lctx : hdr[ 0 ] == -2 ? rm_rctx : &rm_descr[ hdr[ 0 ] ];
		if( stp == NULL )
			die( "seq= of a context that is not there in", fname );
		set_seq( stp, seq );
	}
	/* every expression the blob knows has come with its string, and no other */
	for( i = 0; i < p->n_elems; i++ )
		if( ( p->elems[ i ].re >= 0 ) != ( rm_descr[ i ].s_seq != NULL ) )
			die( "seq= strings do not match the program's in", fname );
	fclose( fp );
	free( p );
}

static	void	mk_rcmp( int slen, char sbuf[] )	/* rnamot.c:193-216, restated */
{
	static	char	wc[ 256 ];
	int	i, j;
	char	c;

	if( !wc[ 0 ] ){
		memset( wc, 'n', sizeof( wc ) );
		wc[ 'a' ] = wc[ 'A' ] = 't';
		wc[ 'c' ] = wc[ 'C' ] = 'g';
		wc[ 'g' ] = wc[ 'G' ] = 'c';
		wc[ 't' ] = wc[ 'T' ] = wc[ 'u' ] = wc[ 'U' ] = 'a';
	}
	for( i = 0, j = slen - 1; i <= j; i++, j-- ){
		c = wc[ ( unsigned char )sbuf[ i ] ];
		sbuf[ i ] = wc[ ( unsigned char )sbuf[ j ] ];
		sbuf[ j ] = c;
	}
}

int	main( int argc, char *argv[] )
{
	FILE	*fp;
	char	*line = NULL, sid[ 32 ], sdef[ 4 ] = "";
	size_t	s_line = 0;
	ssize_t	n;
	int	a = 1;

	if( a < argc && !strcmp( argv[ a ], "-z" ) ){
		fill_byte = 0;
		a++;
	}
	if( argc - a != 2 ){
		fprintf( stderr, "usage: %s [-z] program-file sequence-file\n", argv[ 0 ] );
		return( 2 );
	}
	STREL_T	*volatile aliased = rm_descr;	/* (volatile: two array names never compare equal at compile time) */

	if( aliased != drv_descr_store + 1 ){		/* the alias above did not take: rm_descr[ -1 ] would not be ours */
		fprintf( stderr, "find_motif_drv: rm_descr is not drv_descr_store + 1\n" );
		return( 2 );
	}
	load_program( argv[ a ] );
	if( RM_fm_init() )
		return( 1 );
	if( ( fp = fopen( argv[ a + 1 ], "r" ) ) == NULL )
		die( "can't read", argv[ a + 1 ] );
	for( cur_entry = 0; ( n = getline( &line, &s_line, fp ) ) >= 0; cur_entry++ ){
		int	slen = ( int )n;
		if( slen > 0 && line[ slen - 1 ] == '\n' )
			line[ --slen ] = '\0';
		sprintf( sid, "e%d", cur_entry );
		RM_find_motif( rm_n_searches, rm_searches, rm_sites, sid, sdef, 0, slen, line );
		if( args.a_copt ){
			mk_rcmp( slen, line );
				RM_find_motif( rm_n_searches, rm_searches, rm_sites, sid, sdef, 1, slen, line );
		}
	}
	fclose( fp );
	return( 0 );
}
