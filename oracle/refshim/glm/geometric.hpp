// Stand-in for <glm/geometric.hpp>: the whole subset lives in one header.
#pragma once
#include "rt2_glm.hpp"
