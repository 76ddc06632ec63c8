// tests/hostsim/own_check.cpp -- TEST INFRASTRUCTURE, not product code.
//
// The owners of rnamotif_amd/csrc/rm_hip_own.h against a counting fake of the runtime: this file defines the ten calls
// of the runtime the header makes, over malloc, with a count of what is alive, a record of every call and a call number
// at which the next allocation or creation fails.  No device, no ROCm library.  tests/test_hip_own_cpu.py builds and
// runs it, once more with -fsanitize=address,undefined.  Exit status 0 and "own_check: ok" when every check holds;
// otherwise a line per failed check on stderr and exit status 1.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>
#include "rm_hip_own.h"

// ---------------------------------------------------------------- the fake
static int	g_live = 0;			// memory, streams and events that are alive
static int	g_calls = 0, g_fail_at = -1;	// allocations and creations so far; the one that fails (-1: none)
static int	g_bad_free = 0;			// frees and destroys of what was not alive
static size_t	g_asked = 0;			// bytes of the last allocation
static std::set<void *>	g_alive;
static std::vector<std::string>	g_log;		// "sync" / "destroy" of streams, in order

static void *make( size_t bytes )
{
	void	*p = malloc( bytes ? bytes : 1 );
	g_alive.insert( p );
	g_live++;
	return p;
}
static hipError_t unmake( void *p )
{
	if( p == nullptr )
		return hipSuccess;
	if( g_alive.erase( p ) != 1 ){
		g_bad_free++;
		return hipErrorInvalidValue;
	}
	g_live--;
	free( p );
	return hipSuccess;
}
static bool fails() { return g_calls++ == g_fail_at; }

extern "C" {
hipError_t hipMalloc( void **p, size_t bytes )
{
	if( fails() )
		return hipErrorOutOfMemory;
	g_asked = bytes;
	*p = make( bytes );
	return hipSuccess;
}
hipError_t hipHostMalloc( void **p, size_t bytes, unsigned )
{
	if( fails() )
		return hipErrorOutOfMemory;
	g_asked = bytes;
	*p = make( bytes );
	return hipSuccess;
}
hipError_t hipFree( void *p ) { return unmake( p ); }
hipError_t hipHostFree( void *p ) { return unmake( p ); }
hipError_t hipEventCreateWithFlags( hipEvent_t *e, unsigned )
{
	if( fails() )
		return hipErrorOutOfMemory;
	*e = static_cast<hipEvent_t>( make( 1 ) );
	return hipSuccess;
}
hipError_t hipEventDestroy( hipEvent_t e ) { return unmake( e ); }
hipError_t hipStreamCreateWithFlags( hipStream_t *s, unsigned )
{
	if( fails() )
		return hipErrorOutOfMemory;
	*s = static_cast<hipStream_t>( make( 1 ) );
	return hipSuccess;
}
hipError_t hipStreamSynchronize( hipStream_t s )
{
	g_log.push_back( g_alive.count( s ) ? "sync" : "sync of a dead stream" );
	return hipSuccess;
}
hipError_t hipStreamDestroy( hipStream_t s )
{
	g_log.push_back( "destroy" );
	return unmake( s );
}
const char *hipGetErrorString( hipError_t ) { return "fake"; }
}

// ---------------------------------------------------------------- the checks
static int	g_failed = 0;
#define CHECK( cond )	do{ if( !( cond ) ){ fprintf( stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond ); g_failed++; } }while( 0 )

static const size_t	SIZES[] = { 0, 1, 255, 256, 257, size_t( 1 ) << 20 };
static const int	N_SIZES = int( sizeof( SIZES ) / sizeof( SIZES[ 0 ] ) );

// room(): rising then falling sizes; the capacity never shrinks, a fit keeps the pointer, growth asks for want + want / 4
template<class M> static void check_room()
{
	M	m;
	CHECK( !m && m.bytes() == 0 && m.template as<char>() == nullptr );
	for( int pass = 0; pass < 2; pass++ )
		for( int k = 0; k < N_SIZES; k++ ){
			const size_t	want = SIZES[ pass == 0 ? k : N_SIZES - 1 - k ], before = m.bytes();
			void	*was = m.template as<void>();
			const int	calls = g_calls;
			CHECK( m.room( want ) == hipSuccess );
			CHECK( m.bytes() >= want && m.bytes() >= before );
			if( want <= before ){
				CHECK( m.template as<void>() == was && m.bytes() == before && g_calls == calls );
			}else{
				CHECK( g_calls == calls + 1 && g_asked == want + want / 4 && m.bytes() == want + want / 4 );
				CHECK( bool( m ) && g_alive.count( m.template as<void>() ) == 1 );
			}
		}
	CHECK( g_live == 1 );
	// exact(): that size, larger or smaller than what was there
	CHECK( m.exact( 100 ) == hipSuccess && m.bytes() == 100 && g_asked == 100 && g_live == 1 );
	CHECK( m.exact( 1000 ) == hipSuccess && m.bytes() == 1000 && g_asked == 1000 && g_live == 1 );
}

// a failed room() or exact() leaves the owner empty; a later one works; nothing is freed twice
template<class M> static void check_failure()
{
	const int	live = g_live;
	M	m;
	g_fail_at = g_calls;
	CHECK( m.room( 256 ) != hipSuccess && !m && m.bytes() == 0 && g_live == live );
	CHECK( m.room( 256 ) == hipSuccess && bool( m ) && m.bytes() == 320 && g_live == live + 1 );
	g_fail_at = g_calls;
	CHECK( m.room( 4096 ) != hipSuccess && !m && m.bytes() == 0 && m.template as<void>() == nullptr && g_live == live );
	CHECK( m.room( 16 ) == hipSuccess && m.bytes() == 20 && g_live == live + 1 );
	g_fail_at = g_calls;
	CHECK( m.exact( 64 ) != hipSuccess && !m && m.bytes() == 0 && g_live == live );
	CHECK( m.exact( 64 ) == hipSuccess && m.bytes() == 64 && g_live == live + 1 );
	g_fail_at = -1;
	m.reset();
	CHECK( !m && m.bytes() == 0 && g_live == live );
	m.reset();
	CHECK( g_bad_free == 0 );
}

template<class M> static void check_move()
{
	const int	live = g_live;
	M	a;
	CHECK( a.exact( 48 ) == hipSuccess );
	void	*p = a.template as<void>();
	M	b( std::move( a ) );
	CHECK( !a && a.bytes() == 0 && b.template as<void>() == p && b.bytes() == 48 );
	M	c;
	CHECK( c.exact( 8 ) == hipSuccess && g_live == live + 2 );
	c = std::move( b );		// (what c held goes)
	CHECK( !b && b.bytes() == 0 && c.template as<void>() == p && c.bytes() == 48 && g_live == live + 1 );
	M	&self = c;
	c = std::move( self );
	CHECK( c.template as<void>() == p && c.bytes() == 48 && g_live == live + 1 && g_alive.count( p ) == 1 );
}

static void check_stream_and_event()
{
	const int	live = g_live;
	{
		rma::Stream	s;
		CHECK( s.get() == nullptr );
		g_fail_at = g_calls;
		CHECK( s.create( 0 ) != hipSuccess && s.get() == nullptr && g_live == live );
		g_fail_at = -1;
		CHECK( s.create( 0 ) == hipSuccess && s.get() != nullptr && g_live == live + 1 );
		rma::Stream	t( std::move( s ) );
		CHECK( s.get() == nullptr && t.get() != nullptr );
		rma::Stream	&self = t;
		t = std::move( self );
		CHECK( t.get() != nullptr && g_live == live + 1 );
		g_log.clear();
	}
	// the one stream: synchronised, then destroyed; the empty one: neither
	CHECK( g_log.size() == 2 && g_log[ 0 ] == "sync" && g_log[ 1 ] == "destroy" );
	CHECK( g_live == live );
	{
		rma::Event	e;
		g_fail_at = g_calls;
		CHECK( e.create( 0 ) != hipSuccess && e.get() == nullptr && g_live == live );
		g_fail_at = -1;
		CHECK( e.create( 0 ) == hipSuccess && e.get() != nullptr && g_live == live + 1 );
		rma::Event	f;
		f = std::move( e );
		CHECK( e.get() == nullptr && f.get() != nullptr && g_live == live + 1 );
		rma::Event	&self = f;
		f = std::move( self );
		CHECK( f.get() != nullptr && g_live == live + 1 );
	}
	CHECK( g_live == live && g_bad_free == 0 );
}

// a first use as rm_hitpost.cpp writes it: built in locals, moved into the holder when complete
struct Target {
	rma::DevMem	table;
	rma::PinMem	words;
	rma::Event	done;
};
#define TRY( call )	do{ if( ( call ) != hipSuccess ) return 1; }while( 0 )
static int set_up( Target &t )
{
	rma::DevMem	table;
	rma::PinMem	words;
	rma::Event	done;
	TRY( table.exact( 4096 ) );
	TRY( words.exact( 256 ) );
	TRY( done.create( 0 ) );
	t.table = std::move( table );
	t.words = std::move( words );
	t.done = std::move( done );
	return 0;
}

static void check_build_then_commit()
{
	const int	live = g_live;
	Target	t;
	for( int k = 0; k < 3; k++ ){
		g_fail_at = g_calls + k;
		CHECK( set_up( t ) == 1 );
		CHECK( g_live == live );
		CHECK( !t.table && !t.words && t.done.get() == nullptr && t.table.bytes() == 0 && t.words.bytes() == 0 );
	}
	g_fail_at = -1;
	const int	calls = g_calls;
	CHECK( set_up( t ) == 0 && g_calls == calls + 3 );
	CHECK( bool( t.table ) && t.table.bytes() == 4096 && bool( t.words ) && t.words.bytes() == 256 && t.done.get() != nullptr );
	CHECK( g_live == live + 3 );
}

int main()
{
	check_room<rma::DevMem>();
	check_room<rma::PinMem>();
	check_failure<rma::DevMem>();
	check_failure<rma::PinMem>();
	check_move<rma::DevMem>();
	check_move<rma::PinMem>();
	check_stream_and_event();
	check_build_then_commit();
	CHECK( g_live == 0 && g_alive.empty() && g_bad_free == 0 );
	if( g_failed == 0 )
		printf( "own_check: ok\n" );
	return g_failed == 0 ? 0 : 1;
}
