// rm_flight_count.h -- how many scans are in flight on each device of this process, so that a scanner that begins one
// knows whether another scanner's is on its way (rm_scanner.cpp: option beside at -1).  No HIP, no lock: one atomic
// count a device and a mark that a scan holds while it is counted.  tests/hostsim/flight_count_check.cpp runs it from
// eight threads under the thread and address sanitizers.
#pragma once
#include <atomic>

namespace rma {

constexpr int	FLIGHT_DEVICES = 64;		// (device numbers beyond share the last count: the shape of a launch depends on it, no result)

inline std::atomic<int> &flights_of( int device )
{
	static std::atomic<int>	n[ FLIGHT_DEVICES ];	// (zero-initialised)
	return n[ device < 0 ? 0 : device < FLIGHT_DEVICES ? device : FLIGHT_DEVICES - 1 ];
}

// scans in flight on the device, the asking scanner's own included if it holds a mark
inline int flights( int device ) { return flights_of( device ).load( std::memory_order_relaxed ); }

// One scan's place in its device's count: raised once the scan is certain to be launched, lowered when it is done --
// or when the holder goes, whichever way a function is left.  Raising a raised mark and lowering a lowered one do
// nothing, so that every path may lower.  A mark belongs to one scanner, which one thread uses at a time.
class FlightMark {
	std::atomic<int>	*n_ = nullptr;
public:
	FlightMark() = default;
	FlightMark( const FlightMark & ) = delete;
	FlightMark &operator=( const FlightMark & ) = delete;
	~FlightMark() { lower(); }
	bool	raised() const { return n_ != nullptr; }
	void	raise( int device )
	{
		if( n_ == nullptr ){
			n_ = &flights_of( device );
			n_->fetch_add( 1, std::memory_order_relaxed );
		}
	}
	void	lower()
	{
		if( n_ != nullptr ){
			n_->fetch_sub( 1, std::memory_order_relaxed );
			n_ = nullptr;
		}
	}
};

}	// namespace rma
