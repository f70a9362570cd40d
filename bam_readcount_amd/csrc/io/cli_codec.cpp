// cli_codec.cpp — the codec libraries through dlopen (nothing of them is linked: the simulator's command line is these very files):
// the inflater of include/brc_inflate.h behind --brc-device-inflate, the deflater of include/brc_deflate.h behind --brc-bgzf-output.
// A missing library, entry point or device ends the run — there is no quiet return to the host path or to plain text.
#include <dlfcn.h>
#include <limits.h>

#include "cli_internal.h"

// One codec library: where it is (the environment's word as given, else next to this program), its entry points — all of `names`, the
// first of which creates a handle — and a handle on `device`.  *lib, once open, serves the next caller.  Returns 0, or the step that
// failed: 1 no library (said here: both switches word it alike), 2 an entry point is missing, 3 no handle (*rc says why) — those two
// the callers word themselves.
static int load_codec(const char* sw, const char* what, bool given, const std::string& given_path, const char* file, void** lib, std::string* path,
                      const char* const* names, void** fns, size_t n, int device, void** handle, int* rc) {
    if (!*lib) {
        if (given) *path = given_path;
        else {
            char exe[PATH_MAX]; const ssize_t len = readlink("/proc/self/exe", exe, sizeof exe - 1);
            const std::string self = len > 0 ? std::string(exe, (size_t)len) : std::string("bam-readcount");
            const size_t sl = self.rfind('/');
            *path = (sl == std::string::npos ? std::string(".") : self.substr(0, sl)) + "/" + file;
        }
        *lib = dlopen(path->c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!*lib) { fprintf(stderr, "bam-readcount: %s: cannot load the %s library %s: %s\n", sw, what, path->c_str(), dlerror()); return 1; }
    }
    for (size_t i = 0; i < n; ++i) fns[i] = dlsym(*lib, names[i]);
    for (size_t i = 0; i < n; ++i) if (!fns[i]) return 2;
    *handle = nullptr;
    *rc = ((int (*)(int, void**))fns[0])(device, handle);
    return *rc != 0 || !*handle ? 3 : 0;
}

int open_inflater(Ctx& c, int device) {
    static std::mutex mu; std::lock_guard<std::mutex> g(mu);      // (every engine's set-up thread comes here: the library is loaded once)
    static void* lib = nullptr; static std::string path;
    static const char* const names[] = {"brc_inflater_create", "brc_inflate_bgzf"};
    void* fn[2]; void* h = nullptr; int rc = 0;
    switch (load_codec("--brc-device-inflate", "inflater", g_knobs.has_inflate_lib, g_knobs.inflate_lib, "libbrc_inflate_hip.so", &lib, &path, names, fn, 2, device, &h, &rc)) {
        case 0: break;
        case 2: fprintf(stderr, "bam-readcount: --brc-device-inflate: %s does not export the inflater of include/brc_inflate.h\n", path.c_str()); return 1;
        case 3: fprintf(stderr, "bam-readcount: --brc-device-inflate: cannot create an inflater on device %d: %s\n", device, brc_strerror(rc)); return 1;
        default: return 1;
    }
    c.inf = new ExtInflater();
    c.inf->handle = h;
    c.inf->destroy = (void (*)(void*))dlsym(lib, "brc_inflater_destroy");
    c.inf->inflate = (int (*)(void*, const void*, size_t, void*, size_t, uint64_t*, uint8_t*, size_t*))fn[1];
    return 0;
}

// ... and the sink that feeds the deflater (BgzfSink)
int open_bgzf_sink(int device) {
    void* lib = nullptr; std::string path;
    static const char* const names[] = {"brc_deflater_create", "brc_deflate_bgzf", "brc_deflate_bound", "brc_deflate_host_alloc"};
    void* fn[4]; void* h = nullptr; int rc = 0;
    switch (load_codec("--brc-bgzf-output", "deflater", g_knobs.has_deflate_lib, g_knobs.deflate_lib, "libbrc_deflate_hip.so", &lib, &path, names, fn, 4, device, &h, &rc)) {
        case 0: break;
        case 2: fprintf(stderr, "bam-readcount: --brc-bgzf-output: cannot load the deflater library %s: it does not export the deflater of include/brc_deflate.h\n", path.c_str()); return 1;
        case 3: fprintf(stderr, "bam-readcount: --brc-bgzf-output: cannot load the deflater library %s: no deflater on device %d: %s\n", path.c_str(), device, brc_strerror(rc)); return 1;
        default: return 1;
    }
    size_t (*bound)(size_t) = (size_t (*)(size_t))fn[2];
    void* (*halloc)(size_t) = (void* (*)(size_t))fn[3];
    BgzfSink* s = new BgzfSink();
    s->handle = h;
    s->deflate = (int (*)(void*, const void*, size_t, void*, size_t, size_t*, size_t*))fn[1];
    s->last_error = (const char* (*)(const void*))dlsym(lib, "brc_deflater_last_error");
    s->batch = g_knobs.bgzf_batch;          // DESIGN.md 6b (BRC_BGZF_BATCH: bytes; tests cut their kilobytes of text into several calls)
    s->dst_cap = bound(s->batch);
    s->buf[0] = (char*)halloc(s->batch); s->buf[1] = (char*)halloc(s->batch); s->dst = (char*)halloc(s->dst_cap);
    if (!s->buf[0] || !s->buf[1] || !s->dst) { fprintf(stderr, "bam-readcount: --brc-bgzf-output: no page-locked memory for batches of %zu bytes\n", s->batch); return 1; }
    s->worker = std::thread([s]() { s->run(); });
    g_sink = s;
    return 0;
}
