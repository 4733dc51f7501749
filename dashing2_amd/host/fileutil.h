// fileutil.h -- the file and clock helpers the CLI and its ingest pipeline share (POSIX stat, steady clock).
#pragma once
#include <chrono>
#include <string>
#include <sys/stat.h>

namespace d2h {

inline bool isfile(const std::string &p) { struct stat st; return ::stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }
inline size_t filesize(const std::string &p) { struct stat st; return ::stat(p.c_str(), &st) == 0 ? size_t(st.st_size) : 0; }
inline std::string trim_folder(const std::string &s) {   // src/enums.cpp:22-26
    const auto pos = s.find_last_of('/');
    return pos == std::string::npos ? s : s.substr(pos + 1);
}
inline double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace d2h
