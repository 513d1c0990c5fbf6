/* Stand-in for <H5Cpp.h>: the reference never reaches its HDF5 writer from the kernel source. */
#pragma once
