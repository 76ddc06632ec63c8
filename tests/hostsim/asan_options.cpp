// asan_options.cpp -- linked into the sanitized builds of the host checkers alone.  The front end keeps what it parsed for the
// life of the process, as the reference does, so the leak check at exit is off; everything else AddressSanitizer checks is on.
extern "C" const char *__asan_default_options() { return "detect_leaks=0"; }
