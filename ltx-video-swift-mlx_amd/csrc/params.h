// params.h - the parameter table of the transformer-family models (dit, connector, attn_module, dual_block, dual_model): declare
// every parameter once, place them in declaration order in one or two HBM arenas, then load / fill / export by module key. The
// conv-weight models (vae, vae_encoder, upscaler, audio) re-lay their weights on load and keep their own slot types.
#pragma once
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "runtime.h"

struct LinearW;  // dit.h

enum SlotKind { SLOT_BF16 = 0, SLOT_F32 = 1 };
struct ParamSlot {
    // quantised model: the slot of a Linear weight points at its codes / scales / biases instead of dst (rows of a fused matrix
    // are row offsets into all three)
    uint8_t* q = nullptr;
    bf16_t* qs = nullptr;
    bf16_t* qb = nullptr;
    void* dst = nullptr;
    int kind = SLOT_BF16;
    long numel = 0;
    long rows = 0, cols = 0;  // expected shape (cols = 0 -> vector)
    int init = 0;             // 0: zeros, 1: ones (reference initialisers for parameters absent from the file)
    bool loaded = false;
};

struct ParamTable {
    std::map<std::string, ParamSlot> slots;  // module key -> destination
    DeviceArena arena;   // f32 parameters (biases, norm weights, scale-shift tables); everything when place(false)
    DeviceArena warena;  // place(true): the bf16 Linear weights on their own (dit_quantize releases exactly these)

    // Declarations. *dst receives the device pointer in place(). A hidden declaration is placed and gets no key: the fused q|k
    // matrix and the stacked scale-shift tables, which files and callers name only through view()s.
    void add(const std::string& key, void** dst, int kind, long rows, long cols, int init = 0);
    void add_hidden(void** dst, int kind, long rows, long cols) { add("", dst, kind, rows, cols); }
    void add_linear(const std::string& name, LinearW& l, int out, int in);  // sets l.out / l.in; name.weight [out][in] bf16, name.bias [out] f32
    // Reserve and zero the arena(s), take the bytes in declaration order (so consecutive declarations of one kind are contiguous up
    // to the arena's 256-byte grain), fill the slots and the init == 1 parameters. Returns the padded bytes of all parameters.
    size_t place(bool split_weights);
    // a sub-range of a placed parameter under a module key of its own (after place())
    void view(const std::string& key, void* dst, int kind, long rows, long cols);
    const ParamSlot* find(const std::string& key) const {
        auto it = slots.find(key);
        return it == slots.end() ? nullptr : &it->second;
    }

   private:
    struct Decl {
        std::string key;
        void** dst;
        ParamSlot slot;
    };
    std::vector<Decl> decls_;
};

// weightLoadingFailed unless the file tensor has the slot's element count and, when it is 2-D and the slot is a matrix, its [rows, cols]
void param_check_shape(const std::string& file_key, const StTensor& t, const ParamSlot& s);
// One file tensor into its slot: bf16 as it is; an f32 slot keeps the bf16-rounded value in an f32 container, because every
// parameter is cast to bf16 when the reference applies it (ModelDownloader.swift:1005-1012). `staging` is the caller's, reused.
void param_upload(const SafeTensors& st, const StTensor& t, const ParamSlot& s, std::vector<uint8_t>* staging);
// File-driven load. map_key: file key in, false ("not mine") or the module key out. A mapped key without a slot counts as unmatched;
// a slot counts as loaded once however many file keys name it (the later key in map order wins); slots no key named count as
// missing. Resets the load report unless `continue_report`. Returns the first missing key, or empty.
std::string param_table_load(ltx_ctx* ctx, ParamTable& table, const SafeTensors& st,
                             const std::function<bool(const std::string& file_key, std::string* module_key)>& map_key, bool continue_report = false);
// Synthetic weights: slot number k (1-based, map order) is filled from seed * 0x9E3779B97F4A7C15 + (first_counter + k) * 0xD1B54A32D192ED03;
// rule gives an f32 slot's {mean, stddev} and a bf16 slot's stddev (its mean is 0). Values are bf16-representable.
using ParamFillRule = std::function<std::pair<float, float>(const std::string& key, const ParamSlot& slot)>;
void param_table_fill_synthetic(ltx_ctx* ctx, ParamTable& table, uint64_t seed, uint64_t first_counter, const ParamFillRule& rule);
// the rule four of the five models share: weights and tables N(0, 0.02^2), biases N(0, 0.01^2), q / k norm weights 1 + N(0, 0.02^2)
std::pair<float, float> param_fill_rule_default(const std::string& key, const ParamSlot& slot);
// one parameter back to the host as f32 (waits for the context's stream first)
void param_export(ltx_ctx* ctx, const ParamSlot& s, float* out);
