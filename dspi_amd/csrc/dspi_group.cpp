// dspi_group.cpp — see dspi_group.h.
#include "dspi_group.h"

#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>

namespace dspi {

std::vector<uint32_t> group_classes(const ImageSig *sig, size_t n) {
    std::vector<uint32_t> out(n, 0);
    std::unordered_map<std::string, uint32_t> seen;      // the signature's bytes -> the first image that has them
    for (size_t i = 0; i < n; i++)
        out[i] = seen.emplace(std::string(reinterpret_cast<const char *>(&sig[i]), sizeof(ImageSig)), (uint32_t)i).first->second;
    return out;
}

std::vector<StreamMove> group_plan(const uint8_t *active, const int32_t *stream_object, const uint32_t *object_class, uint32_t n_streams, bool one_way) {
    std::vector<StreamMove> out;
    if (!stream_object || n_streams == 0) return out;
    auto is_active = [&](uint32_t s) { return !active || active[s] != 0; };
    // groups: per object its active streams and the lowest of them; per class the lowest of all
    size_t n_objects = 0;
    for (uint32_t s = 0; s < n_streams; s++) n_objects = std::max(n_objects, (size_t)stream_object[s] + 1);
    std::vector<uint32_t> size(n_objects, 0), first(n_objects, kMoveNone);
    std::unordered_map<uint32_t, uint32_t> class_first;
    uint32_t n_active = 0;
    for (uint32_t s = 0; s < n_streams; s++) {
        if (!is_active(s)) continue;
        const size_t o = (size_t)stream_object[s];
        n_active++;
        if (size[o]++ == 0) { first[o] = s; class_first.emplace(object_class ? object_class[o] : 0u, s); }      // (ascending s: the first seen is the lowest)
    }
    std::vector<uint32_t> order;
    for (size_t o = 0; o < n_objects; o++) if (size[o]) order.push_back((uint32_t)o);
    auto key = [&](uint32_t o) { return class_first[object_class ? object_class[o] : 0u]; };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { const uint32_t ka = key(a), kb = key(b); return ka != kb ? ka < kb : first[a] < first[b]; });
    // runs
    std::vector<uint32_t> run(n_objects, 0), next(n_objects, 0);      // next: the lowest slot of the run that may still be free
    uint32_t at = 0;
    for (uint32_t o : order) { run[o] = next[o] = at; at += size[o]; }
    // residents stay; movers fill what the residents leave of their run, both ascending
    auto resident = [&](uint32_t s) { const size_t o = (size_t)stream_object[s]; return is_active(s) && s >= run[o] && s - run[o] < size[o]; };
    for (uint32_t s = 0; s < n_streams; s++) {
        if (!is_active(s) || resident(s)) continue;
        const size_t o = (size_t)stream_object[s];
        while (is_active(next[o]) && (size_t)stream_object[next[o]] == o) next[o]++;      // (a stream of o inside o's run is a resident)
        out.push_back(StreamMove{s, next[o]++});
    }
    // the paused streams below A go where active ones came from
    if (!one_way) {
        uint32_t t = n_active;
        for (uint32_t h = 0; h < n_active; h++) {
            if (is_active(h)) continue;
            while (!is_active(t)) t++;      // (as many active slots at or above A as paused ones below it)
            out.push_back(StreamMove{h, t++});
        }
    }
    std::sort(out.begin(), out.end(), [](const StreamMove &a, const StreamMove &b) { return a.dst < b.dst; });
    return out;
}

}  // namespace dspi
