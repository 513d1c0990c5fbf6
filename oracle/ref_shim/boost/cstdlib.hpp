/* Stand-in for <boost/cstdlib.hpp>: nothing of it is used by the kernel source. */
#pragma once
