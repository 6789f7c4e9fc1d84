// Stand-in for Boost.Log's trivial logger, written from its public names only (oracle/ref_shim/README.md): a stream that discards.
#pragma once
#include <iostream>
#define BOOST_LOG_ATTRIBUTE_KEYWORD(keyword, name, type) struct keyword##_stand_in
namespace boost {
namespace log {
struct null_stream {
    template <class T> null_stream& operator<<(const T&) { return *this; }
};
namespace trivial {
enum severity_level { trace, debug, info, warning, error, fatal };
struct logger {
    static int get() { return 0; }
};
}  // namespace trivial
namespace keywords {
struct severity_keyword {
    int operator=(int v) const { return v; }
};
static const severity_keyword severity{};
}  // namespace keywords
inline int add_value(const char*, ...) { return 0; }
}  // namespace log
}  // namespace boost
#define BOOST_LOG_STREAM_WITH_PARAMS(logger, params) ::boost::log::null_stream()
