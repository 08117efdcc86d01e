// ref_prelude.hpp — force-included in place of the reference's precompiled header when the reference build
// (oracle/Makefile, target ref) compiles the reference's src/cpu_raytrace in place. TEST INFRASTRUCTURE ONLY.
//
// It includes what the precompiled header includes (without GL) and then renames the three <random> names
// that the reference's RandReal() spells (Math.hpp:9-13), so that RandReal() returns the next float of
// rt2_ref_uniform(), which ref_driver.cpp defines (a Philox4x32-10 stream with the oracle's keying). The
// replacement types live in namespace std because the reference writes std:: in front of each name.
#pragma once

#include <algorithm>
#include <array>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <execution>
#include <functional>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <numbers>
#include <optional>
#include <random>
#include <span>
#include <sstream>
#include <stack>
#include <string>
#include <string_view>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <variant>
#include <vector>

#include <glm/geometric.hpp>
#include <glm/vec2.hpp>
#include <glm/vec3.hpp>
#include <glm/vec4.hpp>

#include "EAssert.hpp"

extern "C" float rt2_ref_uniform();

namespace std {
struct rt2_hook_device {
  unsigned operator()() const { return 0u; }
};
struct rt2_hook_engine {
  explicit rt2_hook_engine(unsigned) {}
};
template <typename T>
struct rt2_hook_distribution {
  rt2_hook_distribution(T, T) {}
  template <typename G>
  T operator()(G&) const {
    return static_cast<T>(rt2_ref_uniform());
  }
};
}  // namespace std

#define random_device rt2_hook_device
#define minstd_rand rt2_hook_engine
#define uniform_real_distribution rt2_hook_distribution
