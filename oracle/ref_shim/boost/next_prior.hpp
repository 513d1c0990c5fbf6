/* Stand-in for <boost/next_prior.hpp>: nothing of it is used by the kernel source. */
#pragma once
