// rm_seqcheck.cpp -- see rm_seqcheck.h: the loose seq= expressions of a compiled descriptor as an image, and what is refused.
#include "rm_host.h"
#include "rm_regex.h"
#include "rm_seqcheck.h"
#include <atomic>
#include <cstdio>
#include <cstring>

namespace rma {

std::string seqcheck_image_make( const Descriptor &d, const rma_program_t &prog, SeqImage *out )
{
	static std::atomic<uint64_t>	serials{ 0 };
	const std::string	who = "the seq= expressions cannot be applied on the device: ";
	char	buf[ 256 ];
	if( int( d.descr.size() ) != prog.n_elems )
		return who + "the program is not this descriptor's";
	RmqImage	hdr;
	memset( &hdr, 0, sizeof( hdr ) );
	hdr.magic = RMQ_MAGIC;
	hdr.stride = rma_hit_stride( &prog );
	std::vector<RmqOp>	ops;
	for( int e = 0; e < prog.n_elems; e++ ){
		const int	ri = prog.elems[ e ].re;
		if( ri < 0 || !prog.regexes[ ri ].loose )
			continue;
		const Strel	&s = d.descr[ size_t( e ) ];
		if( s.re == nullptr || s.seq == nullptr )
			return who + "the program is not this descriptor's";
		if( hdr.n_expr >= RMQ_MAX_EXPR ){
			snprintf( buf, sizeof( buf ), "more than %d elements have a loose seq=", int( RMQ_MAX_EXPR ) );
			return who + buf;
		}
		if( s.re->ops.size() > size_t( RMQ_MAX_OPS ) ){
			snprintf( buf, sizeof( buf ), "element %d's seq= has %zu ops, the image holds %d an expression", e, s.re->ops.size(), int( RMQ_MAX_OPS ) );
			return who + buf;
		}
		RmqExpr	&ex = hdr.expr[ hdr.n_expr++ ];
		ex.elem = e;
		ex.anchored = *s.seq == '^';
		ex.mismatch = s.mismatch;
		ex.first = int32_t( ops.size() );
		ex.n_ops = int32_t( s.re->ops.size() );
		int	repeats = 0;
		if( !rmq_flatten( *s.re, &ops, &repeats ) )
			return who + "a group number beyond 9";
		if( repeats > hdr.frames )
			hdr.frames = repeats;
	}
	hdr.n_ops = int32_t( ops.size() );
	const size_t	bytes = sizeof( RmqImage ) + ops.size() * sizeof( RmqOp );
	const int	cap = bytes > size_t( RMQ_LDS_BYTES ) ? -1 : rmq_frames_cap( int( bytes ) );
	if( cap < 0 ){
		snprintf( buf, sizeof( buf ), "the image of %d ops (%zu bytes) leaves no room in %d bytes of LDS for a wave", hdr.n_ops, bytes, int( RMQ_LDS_BYTES ) );
		return who + buf;
	}
	if( hdr.frames > cap ){
		snprintf( buf, sizeof( buf ), "an expression has %d repeating ops, a wave has room for %d frames next to the image", hdr.frames, cap );
		return who + buf;
	}
	hdr.bytes = int32_t( bytes );
	SeqImage	&img = *out;
	img.blob.assign( bytes / 8, 0 );
	memcpy( img.blob.data(), &hdr, sizeof( hdr ) );
	if( !ops.empty() )
		memcpy( reinterpret_cast<char *>( img.blob.data() ) + sizeof( hdr ), ops.data(), ops.size() * sizeof( RmqOp ) );
	img.prog.reset( new rma_program_t );
	memcpy( img.prog.get(), &prog, sizeof( rma_program_t ) );
	img.serial = ++serials;
	return "";
}

}	// namespace rma
