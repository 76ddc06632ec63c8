// tests/hostsim/diag_slots.cpp -- TEST INFRASTRUCTURE: the counter slots of rm_diag.h as the compiler sees
// them.  tests/test_diag_names.py builds it with -DSLOTS="SLOT( COUNT ) ... EXTENT( PHASES ) ..." and reads "NAME value" lines.
#include <cstdio>
#include "rm_diag.h"
#define SLOT( name_ )	printf( #name_ " %d\n", int( RMK_C_##name_ ) );
#define EXTENT( name_ )	printf( "N_" #name_ " %d\n", int( RMK_CN_##name_ ) );
int main()
{
	printf( "N_COUNTERS %d\nGCTL %d\n", RMK_N_COUNTERS, RMK_GCTL );
	SLOTS
	return 0;
}
