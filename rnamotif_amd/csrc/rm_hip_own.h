// rm_hip_own.h -- what the host files behind the C ABI hold on a GPU, owned by type: device memory, page-locked memory,
// streams and events.  Each owner frees what it holds when it goes, moves and does not copy.  Beside DevCtx's cache of
// database blocks (rm_scanner.cpp) nothing else in csrc/ allocates from or gives back to the runtime.
//
// Memory is a pointer and its capacity in bytes, which change together or not at all: after a failed room() or exact()
// the owner is empty -- null, 0 bytes -- never a pointer with the capacity of another.
//
// An owner waits for nobody but Stream, which synchronises before it is destroyed.  Work that may still touch a buffer
// is the holder's to wait for before the buffer goes (the rule is stated in rm_scanner_impl.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <utility>

namespace rma {

class Mem {
public:
	Mem( const Mem & ) = delete;
	Mem &operator=( const Mem & ) = delete;
	// room for `want` bytes: what is there, or a new piece a quarter larger (what was there is freed first, not copied)
	hipError_t	room( size_t want ) { return want <= cap_ ? hipSuccess : exact( want + want / 4 ); }
	// a new piece of exactly `bytes`, whatever was there
	hipError_t	exact( size_t bytes )
	{
		reset();
		void	*q = nullptr;
		const hipError_t	e = pinned_ ? hipHostMalloc( &q, bytes, hipHostMallocDefault ) : hipMalloc( &q, bytes );
		if( e == hipSuccess ){
			p_ = q;
			cap_ = bytes;
		}
		return e;
	}
	void	reset()
	{
		if( p_ != nullptr )
			( void )( pinned_ ? hipHostFree( p_ ) : hipFree( p_ ) );
		p_ = nullptr;
		cap_ = 0;
	}
	template<class T> T	*as() const { return static_cast<T *>( p_ ); }
	size_t	bytes() const { return cap_; }
	explicit operator bool() const { return p_ != nullptr; }
protected:
	explicit Mem( bool pinned ) : pinned_( pinned ) {}
	Mem( Mem &&o ) noexcept : p_( o.p_ ), cap_( o.cap_ ), pinned_( o.pinned_ ) { o.p_ = nullptr; o.cap_ = 0; }
	~Mem() { reset(); }
	void	take( Mem &o )
	{
		if( this == &o )
			return;
		reset();
		p_ = o.p_;
		cap_ = o.cap_;
		o.p_ = nullptr;
		o.cap_ = 0;
	}
private:
	void	*p_ = nullptr;
	size_t	cap_ = 0;
	bool	pinned_;
};

struct DevMem : Mem {		// hipMalloc / hipFree
	DevMem() : Mem( false ) {}
	DevMem( DevMem &&o ) noexcept : Mem( std::move( o ) ) {}
	DevMem &operator=( DevMem &&o ) noexcept { take( o ); return *this; }
};

struct PinMem : Mem {		// hipHostMalloc / hipHostFree
	PinMem() : Mem( true ) {}
	PinMem( PinMem &&o ) noexcept : Mem( std::move( o ) ) {}
	PinMem &operator=( PinMem &&o ) noexcept { take( o ); return *this; }
};

class Stream {
public:
	Stream() = default;
	Stream( Stream &&o ) noexcept : s_( o.s_ ) { o.s_ = nullptr; }
	Stream &operator=( Stream &&o ) noexcept { if( this != &o ){ reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
	~Stream() { reset(); }
	hipError_t	create( unsigned flags )
	{
		reset();
		hipStream_t	s = nullptr;
		const hipError_t	e = hipStreamCreateWithFlags( &s, flags );
		if( e == hipSuccess )
			s_ = s;
		return e;
	}
	hipStream_t	get() const { return s_; }
private:
	void	reset()
	{
		if( s_ != nullptr ){
			( void )hipStreamSynchronize( s_ );
			( void )hipStreamDestroy( s_ );
		}
		s_ = nullptr;
	}
	hipStream_t	s_ = nullptr;
};

class Event {
public:
	Event() = default;
	Event( Event &&o ) noexcept : e_( o.e_ ) { o.e_ = nullptr; }
	Event &operator=( Event &&o ) noexcept { if( this != &o ){ reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
	~Event() { reset(); }
	hipError_t	create( unsigned flags )
	{
		reset();
		hipEvent_t	v = nullptr;
		const hipError_t	e = hipEventCreateWithFlags( &v, flags );
		if( e == hipSuccess )
			e_ = v;
		return e;
	}
	hipEvent_t	get() const { return e_; }
private:
	void	reset()
	{
		if( e_ != nullptr )
			( void )hipEventDestroy( e_ );
		e_ = nullptr;
	}
	hipEvent_t	e_ = nullptr;
};

}	// namespace rma
