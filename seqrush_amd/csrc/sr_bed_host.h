// sr_bed_host.h -- the BED line reader the stages that take intervals share (lift, extract; DESIGN.md section 17 "the BED
// lines"): which lines are skipped, how a line is split, what a number is, and the two refusals that name their line.  The
// stage's prefix is a parameter, so "lift: BED line n: ..." keeps its bytes.  Host only, header only (a stage's .hip file is
// also compiled alone).  What a stage does with a name, a range and a label is its own business: on_line.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_sort.h"

// a decimal number below 2^64, digits only
inline bool sr_bed_number(const std::string &f, uint64_t *out) {
    if (f.empty()) return false;
    uint64_t x = 0;
    for (char c : f) {
        if (c < '0' || c > '9') return false;
        const uint64_t d = (uint64_t)(c - '0');
        if (x > (~0ULL - d) / 10) return false;
        x = x * 10 + d;
    }
    *out = x;
    return true;
}

inline bool sr_bed_starts(const std::string &s, const char *w) { return s.compare(0, strlen(w), w) == 0; }

// Every line that is not blank, a comment, a track or a browser line: split at tabs if it has one, else at blanks, into at
// most four fields (the fourth is the label; with blanks it ends at the next blank, with tabs at the next tab); a CR before
// the newline is dropped.  Fewer than three fields or a start / end that is no number: SR_ERR_INVALID with the line number.
// on_line(f, start, end) -> a status; the first that is not SR_OK ends the reading.
template <class F> int sr_bed_lines(const char *bed, const char *prefix, F &&on_line) {
    const char *at = bed;
    for (uint64_t line_no = 1; *at; line_no++) {
        const char *nl = strchr(at, '\n');
        std::string line(at, nl ? (size_t)(nl - at) : strlen(at));
        at = nl ? nl + 1 : at + line.size();
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.find_first_not_of(" \t") == std::string::npos) continue;
        if (line[0] == '#' || sr_bed_starts(line, "track") || sr_bed_starts(line, "browser")) continue;
        std::vector<std::string> f;
        if (line.find('\t') != std::string::npos) {
            for (size_t a = 0; f.size() < 4;) {
                const size_t b = line.find('\t', a);
                f.push_back(line.substr(a, b == std::string::npos ? b : b - a));
                if (b == std::string::npos) break;
                a = b + 1;
            }
        } else {
            for (size_t a = line.find_first_not_of(' '); a != std::string::npos && f.size() < 4;) {
                const size_t b = line.find(' ', a);
                f.push_back(line.substr(a, b == std::string::npos ? b : b - a));
                a = b == std::string::npos ? b : line.find_first_not_of(' ', b);
            }
        }
        const std::string where = std::string(prefix) + ": BED line " + std::to_string(line_no) + ": ";
        if (f.size() < 3) return sr_fail(SR_ERR_INVALID, where + "fewer than three fields");
        uint64_t start = 0, end = 0;
        if (!sr_bed_number(f[1], &start)) return sr_fail(SR_ERR_INVALID, where + "start '" + f[1] + "' is not a number");
        if (!sr_bed_number(f[2], &end)) return sr_fail(SR_ERR_INVALID, where + "end '" + f[2] + "' is not a number");
        if (const int r = on_line(f, start, end)) return r;
    }
    return SR_OK;
}
