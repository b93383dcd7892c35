// boost/functional/hash.hpp -- the one name the search headers planner_manager.h pulls in use; nothing here is called
#ifndef COLLIDE_GOLDEN_BOOST_HASH_HPP_
#define COLLIDE_GOLDEN_BOOST_HASH_HPP_
#include <cstddef>
#include <functional>
namespace boost {
template <class T>
inline void hash_combine(std::size_t& seed, const T& v) {
  seed ^= std::hash<T>()(v) + 0x9e3779b9 + (seed << 6) + (seed >> 2);
}
}  // namespace boost
#endif
