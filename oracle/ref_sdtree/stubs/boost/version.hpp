// Stand-in for <boost/version.hpp>: the reference's headers only test the version number.
#pragma once
#define BOOST_VERSION 105400
