/* Stand-in for <boost/array.hpp>: nothing of it is used by the kernel source. */
#pragma once
