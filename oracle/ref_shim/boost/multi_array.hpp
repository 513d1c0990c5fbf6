/* Stand-in for <boost/multi_array.hpp>: def.cuh only names the type and its index typedef. */
#pragma once
namespace boost {
template <class T, int N>
struct multi_array {
    typedef long index;
};
}
