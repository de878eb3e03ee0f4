// Stand-in for <boost/filesystem/fstream.hpp>.
#pragma once
#include <fstream>
namespace boost { namespace filesystem {
typedef std::ifstream ifstream;
typedef std::ofstream ofstream;
typedef std::fstream fstream;
} }
