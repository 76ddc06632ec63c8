// tests/hostsim/carve_check.cpp -- TEST INFRASTRUCTURE, not product code.
//
// Where rm_hitpost.cpp's scratch arrays lie (rnamotif_amd/csrc/rm_hitpost.h, carved with rm_scanner_impl.h's Carver),
// printed for tests/test_carve_cpu.py, which holds them to the offsets written out by hand.  No device, no HIP call.
//
//   carve_check <chunk> (<n> <row>)...
//   win <chunk> <d_lo d_len d_off d_src d_bad d_tab total> <h_off h_lo h_bad h_tab total>
//   prune <n> <row> <parts> <hdr rows bflag part part_x blocks total>       one line per ( n, row )
//
// Every block is carved twice, as the library does: from a null base (the offsets, the size) and from a base, where each
// array must lie at the base plus its offset (exit status 1 otherwise).
#include <cstdio>
#include <cstdlib>
#include "rm_hitpost.h"

static bool	g_ok = true;

template<class T> static size_t off( const T *p ) { return size_t( reinterpret_cast<uintptr_t>( p ) ); }

// p, carved from `base`, lies `at` bytes into it
template<class T> static void placed( const T *p, void *base, size_t at, const char *what )
{
	if( reinterpret_cast<uintptr_t>( p ) != reinterpret_cast<uintptr_t>( base ) + at ){
		fprintf( stderr, "%s: carved from a base it does not lie at the base + %zu\n", what, at );
		g_ok = false;
	}
}

int main( int argc, char **argv )
{
	if( argc < 2 || argc % 2 != 0 ){
		fprintf( stderr, "usage: carve_check <chunk> (<n> <row>)...\n" );
		return 2;
	}
	void	*base = reinterpret_cast<void *>( uintptr_t( 0x7f0000001000ull ) );	// (never read)
	const size_t	chunk = size_t( atoll( argv[ 1 ] ) );
	rma::HitWinFixed	f, g;
	const size_t	dev = f.carve_dev( nullptr, chunk ), host = f.carve_host( nullptr, chunk );
	printf( "win %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", chunk, off( f.d_lo ), off( f.d_len ), off( f.d_off ), off( f.d_src ),
		off( f.d_bad ), off( f.d_tab ), dev, off( f.h_off ), off( f.h_lo ), off( f.h_bad ), off( f.h_tab ), host );
	if( g.carve_dev( base, chunk ) != dev || g.carve_host( base, chunk ) != host )
		g_ok = false;
	placed( g.d_lo, base, off( f.d_lo ), "d_lo" ); placed( g.d_len, base, off( f.d_len ), "d_len" ); placed( g.d_off, base, off( f.d_off ), "d_off" );
	placed( g.d_src, base, off( f.d_src ), "d_src" ); placed( g.d_bad, base, off( f.d_bad ), "d_bad" ); placed( g.d_tab, base, off( f.d_tab ), "d_tab" );
	placed( g.h_off, base, off( f.h_off ), "h_off" ); placed( g.h_lo, base, off( f.h_lo ), "h_lo" ); placed( g.h_bad, base, off( f.h_bad ), "h_bad" );
	placed( g.h_tab, base, off( f.h_tab ), "h_tab" );
	for( int a = 2; a + 1 < argc; a += 2 ){
		const size_t	n = size_t( atoll( argv[ a ] ) ), row = size_t( atoll( argv[ a + 1 ] ) ), parts = size_t( rma::prune_parts( int64_t( n ) ) );
		rma::PruneDev	p, q;
		const size_t	total = rma::prune_carve( p, nullptr, n, parts, row );
		printf( "prune %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", n, row, parts, off( p.hdr ), off( p.rows ), off( p.bflag ), off( p.part ),
			off( p.part_x ), off( p.blocks ), total );
		if( rma::prune_carve( q, base, n, parts, row ) != total )
			g_ok = false;
		placed( q.hdr, base, off( p.hdr ), "hdr" ); placed( q.rows, base, off( p.rows ), "rows" ); placed( q.bflag, base, off( p.bflag ), "bflag" );
		placed( q.part, base, off( p.part ), "part" ); placed( q.part_x, base, off( p.part_x ), "part_x" ); placed( q.blocks, base, off( p.blocks ), "blocks" );
	}
	return g_ok ? 0 : 1;
}
