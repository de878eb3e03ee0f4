// Stand-in for <boost/scoped_ptr.hpp>: enough for the declarations in the reference's headers (nothing here is ever called).
#pragma once
namespace boost {
template <class T> class scoped_ptr {
    T *p;
public:
    explicit scoped_ptr(T *q = 0) : p(q) {}
    T *get() const { return p; }
    T *operator->() const { return p; }
    T &operator*() const { return *p; }
    void reset(T *q = 0) { p = q; }
};
}
