/* Silences std::cout for the lifetime of the object (the reference prints per call, one of its functions per pixel)
 * and puts the stream's buffer back afterwards. */
#ifndef DCMT_REFBUILD_QUIET_H
#define DCMT_REFBUILD_QUIET_H
#include <iostream>
#include <streambuf>
namespace refbuild {
class Quiet {
    struct Sink : std::streambuf {
        int_type overflow(int_type c) override { return traits_type::not_eof(c); }
        std::streamsize xsputn(const char *, std::streamsize n) override { return n; }
    } sink_;
    std::streambuf *saved_;
public:
    Quiet() : saved_(std::cout.rdbuf(&sink_)) {}
    ~Quiet() { std::cout.rdbuf(saved_); }
    Quiet(const Quiet &) = delete;
    Quiet &operator=(const Quiet &) = delete;
};
}  // namespace refbuild
#endif
