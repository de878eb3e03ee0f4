// Stand-in for <boost/filesystem.hpp>: enough for the declarations in the reference's headers (nothing here is ever called).
#pragma once
#include <string>
namespace boost { namespace filesystem {
class path {
    std::string s;
public:
    path() {}
    path(const std::string &x) : s(x) {}
    path(const char *x) : s(x) {}
    std::string string() const { return s; }
    path parent_path() const { return *this; }
    path filename() const { return *this; }
    path extension() const { return *this; }
    path operator/(const path &o) const { return path(s + "/" + o.s); }
    bool empty() const { return s.empty(); }
};
} }
