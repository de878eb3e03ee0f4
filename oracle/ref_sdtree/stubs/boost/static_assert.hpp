// Stand-in for <boost/static_assert.hpp>.
#pragma once
#define BOOST_STATIC_ASSERT(x) static_assert(x, #x)
