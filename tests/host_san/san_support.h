// tests/host_san/san_support.h -- what the stand-alone sanitizer programs under tests/*_san/ share: the CHECK macro, the stand-in for a
// device pointer, heap blocks of exactly the size a caller owns, the walker that counts an entry point's calls and checks its refusals,
// and the well-formed arguments of an Adam sequence call.  Each program is one translation unit that includes this once, after the public
// header of the entry point it walks.  tests/test_host_san.py builds and runs them all.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dragposer_sequence_constraints.h"

extern "C" int dp_debug_host_ctx(dp_ctx**); // the library's private hook: a context with no device behind it

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

float* const PTR = (float*)0x10000; // stands for a device pointer: never dereferenced on a context without a device

// a T in a heap block of exactly `size` bytes (default: sizeof(T))
template <class T>
struct Exact {
    void* block;
    explicit Exact(const T& init, size_t size = sizeof(T)) : block(std::malloc(size)) { std::memcpy(block, &init, size < sizeof(T) ? size : sizeof(T)); }
    ~Exact() { std::free(block); }
    Exact(const Exact&) = delete;
    const T* get() const { return (const T*)block; }
};
// the block of a T whose struct_size says `size`: never more than the caller's own sizeof(T)
template <class T>
size_t cut(unsigned size) { return size < sizeof(T) ? size : sizeof(T); }

template <class T>
struct Array { // exactly the vector's entries on the heap (none: a NULL pointer)
    T* p;
    explicit Array(const std::vector<T>& v) : p(v.empty() ? nullptr : (T*)std::malloc(v.size() * sizeof(T)))
    {
        if (p) std::memcpy(p, v.data(), v.size() * sizeof(T));
    }
    ~Array() { std::free(p); }
    Array(const Array&) = delete;
};
// n values of T in a heap block of exactly n * sizeof(T) bytes
template <class T>
struct Block {
    T* p;
    explicit Block(int n) : p((T*)std::malloc((size_t)(n > 0 ? n : 1) * sizeof(T))) {}
    ~Block() { std::free(p); }
    Block(const Block&) = delete;
};

inline bool said(dp_ctx* ctx, const char* word) { return std::string(dp_last_error(ctx)).find(word) != std::string::npos; }

// One program's walk: a host-only context, the entry point whose name every refusal must carry, and the count of calls checked.
struct Walker {
    const char* program;
    const char* entry_point;
    dp_ctx* ctx = nullptr;
    int n = 0;
    Walker(const char* program_, const char* entry_point_) : program(program_), entry_point(entry_point_) { CHECK(dp_debug_host_ctx(&ctx) == DP_OK && ctx); }
    void refused(int rc, const char* word)
    {
        CHECK(rc == DP_ERR_INVALID);
        if (!said(ctx, word)) { std::fprintf(stderr, "expected '%s' in: %s\n", word, dp_last_error(ctx)); std::exit(1); }
        CHECK(said(ctx, entry_point));
        ++n;
    }
    void unsupported(int rc, const char* unit) // well-formed: this link has no kernel unit, which the library says after every argument check
    {
        CHECK(rc == DP_ERR_UNSUPPORTED);
        CHECK(said(ctx, unit));
        ++n;
    }
    void done()
    {
        dp_destroy(ctx);
        std::printf("%s: %d calls, all checks held\n", program, n);
    }
};

// The well-formed arguments that the Adam sequence calls (holds, latent_ar, gaps, tethers, points) build alike.  frames.z_tgt and
// params.lambda_tmp differ between them and stay zero here; a program sets those, and whatever its Case varies, before the hand-over.
struct SeqArgs {
    dp_seq_frames frames{};
    dp_params params = DP_PARAMS_INIT;
    dp_seq_state state{};
    dp_seq_step step{};
    dp_seq_results results = DP_SEQ_RESULTS_INIT;
    dp_seq_extra extra = DP_SEQ_EXTRA_INIT;
    dp_skeleton_in skeleton = DP_SKELETON_IN_INIT;
    SeqArgs()
    {
        frames.n_steps = 3; frames.tgt_pos = frames.tgt_rot = frames.w = PTR; frames.tracked = (const unsigned char*)PTR;
        params.n_iter = 10; params.lr = 1e-2f; params.beta1 = 0.9f; params.beta2 = 0.999f; params.eps = 1e-8f; params.lambda_rot = 1.f;
        state.global_pos = state.global_rot = state.latent_buf = state.disp_buf = state.heights_buf = PTR; state.history = 60; state.n_heights = 2;
        state.height_joints[0] = 4; state.height_joints[1] = 8;
        step.adjust_joint = 0; step.adjust_target_joint = 13; step.adjust_weight = 0.5f;
        results.pose_ret = results.pos_ret = results.loss = results.hist_scratch = PTR;
        extra.loss_terms = extra.joint_pos = PTR;
        skeleton.offsets = PTR; skeleton.stride = DP_SKELETON_STRIDE;
    }
};
// ... each in a heap block of exactly its size
struct SeqBlocks {
    Exact<dp_seq_frames> frames;
    Exact<dp_params> params;
    Exact<dp_seq_state> state;
    Exact<dp_seq_step> step;
    Exact<dp_seq_results> results;
    Exact<dp_seq_extra> extra;
    Exact<dp_skeleton_in> skeleton;
    explicit SeqBlocks(const SeqArgs& a)
        : frames(a.frames), params(a.params), state(a.state), step(a.step), results(a.results), extra(a.extra), skeleton(a.skeleton)
    {
    }
};
