// flight_count_check.cpp -- TEST INFRASTRUCTURE.
//
// rnamotif_amd/csrc/rm_flight_count.h from eight threads: every thread is a scanner that begins and ends scans the ways
// rma_scan_begin() and scan_done() do -- a begin that returns before it raises, one that raises and fails (the guard
// lowers), a scan that runs and is ended twice over, a scanner destroyed with its scan in flight -- while it reads its
// device's count.  The count never leaves 0 .. 8, and is 0 on every device when the threads are through.
// tests/test_beside_plan_cpu.py builds it plain, with -fsanitize=thread and with -fsanitize=address,undefined.
#include <cstdio>
#include <memory>
#include <thread>
#include <vector>
#include "rm_flight_count.h"

static const int	THREADS = 8, ROUNDS = 20000;

// rma_scan_begin's guard: what it lowers on every early return
struct Unfly {
	rma::FlightMark	&m;
	bool	armed;
	~Unfly() { if( armed ) m.lower(); }
};

// 0: the scan is in flight, 1: refused
static int begin( rma::FlightMark &m, int device, int how )
{
	if( how == 0 )		// (refused before the guard is made: a database of another device, a scan already in flight)
		return 1;
	Unfly	unfly{ m, true };
	if( how == 1 )		// (refused while it plans)
		return 1;
	m.raise( device );
	if( how == 2 )		// (the launch failed)
		return 1;
	unfly.armed = false;
	return 0;
}

int main()
{
	const int	devices[ 3 ] = { 0, 3, 1000 };		// (1000: beyond the table, shares the last count)
	std::vector<long long>	bad( THREADS, 0 );
	std::vector<std::thread>	ts;
	for( int t = 0; t < THREADS; t++ )
		ts.emplace_back( [ &, t ]{
			const int	dev = devices[ t % 3 ];
			auto	mark = std::make_unique<rma::FlightMark>();
			for( int i = 0; i < ROUNDS; i++ ){
				const int	how = ( i * 7 + t ) % 5;
				const bool	was = mark->raised();
				const int	rc = begin( *mark, dev, how );
				if( ( rc == 0 ) != ( how >= 3 ) || ( how != 0 && rc != 0 && mark->raised() ) || ( how == 0 && mark->raised() != was ) )
					bad[ t ]++;
				const int	n = rma::flights( dev );
				if( n < ( mark->raised() ? 1 : 0 ) || n > THREADS )
					bad[ t ]++;
				if( how == 3 ){			// scan_done, and once more (rma_scan_end after an error already ended it)
					mark->lower();
					mark->lower();
				}else if( how == 4 )		// the scanner goes with its scan in flight
					mark = std::make_unique<rma::FlightMark>();
				if( mark->raised() )
					bad[ t ]++;
			}
		} );
	for( auto &t : ts )
		t.join();
	long long	n_bad = 0;
	for( long long b : bad )
		n_bad += b;
	for( int d : devices )
		if( rma::flights( d ) != 0 ){
			fprintf( stderr, "device %d: %d scans in flight after the threads\n", d, rma::flights( d ) );
			n_bad++;
		}
	// (two marks raised on one device count two, a mark raised twice one)
	rma::FlightMark	a, b;
	a.raise( 5 );
	a.raise( 5 );
	b.raise( 5 );
	if( rma::flights( 5 ) != 2 )
		n_bad++;
	a.lower();
	b.lower();
	if( rma::flights( 5 ) != 0 )
		n_bad++;
	printf( "flight_count_check: %d threads x %d rounds, %lld violations\n", THREADS, ROUNDS, n_bad );
	return n_bad != 0;
}
