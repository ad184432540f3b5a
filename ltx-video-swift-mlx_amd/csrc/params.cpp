// params.cpp - see params.h.
#include "params.h"

#include "dit.h"

namespace {
size_t slot_bytes(const ParamSlot& s) { return (size_t)s.numel * (s.kind == SLOT_BF16 ? 2 : 4); }

ParamSlot make_slot(void* dst, int kind, long rows, long cols, int init) {
    ParamSlot s;
    s.dst = dst;
    s.kind = kind;
    s.rows = rows;
    s.cols = cols;
    s.numel = rows * (cols ? cols : 1);
    s.init = init;
    return s;
}
}  // namespace

void ParamTable::add(const std::string& key, void** dst, int kind, long rows, long cols, int init) {
    decls_.push_back({key, dst, make_slot(nullptr, kind, rows, cols, init)});
}

void ParamTable::add_linear(const std::string& name, LinearW& l, int out, int in) {
    l.out = out;
    l.in = in;
    add(name + ".weight", (void**)&l.w, SLOT_BF16, out, in);
    add(name + ".bias", (void**)&l.b, SLOT_F32, out, 0);
}

size_t ParamTable::place(bool split_weights) {
    size_t total = 0, total_w = 0;
    for (auto& d : decls_) (split_weights && d.slot.kind == SLOT_BF16 ? total_w : total) += DeviceArena::padded(slot_bytes(d.slot));
    arena.reserve(total + 256);
    HIP_CHECK(hipMemset(arena.buf.p, 0, arena.buf.bytes));
    if (split_weights) {
        warena.reserve(total_w + 256);
        HIP_CHECK(hipMemset(warena.buf.p, 0, warena.buf.bytes));
    }
    for (auto& d : decls_) {
        d.slot.dst = *d.dst = (split_weights && d.slot.kind == SLOT_BF16 ? warena : arena).take(slot_bytes(d.slot));
        // reference initialisers for parameters a file may omit: RMSNorm weights = 1 (LTXAttention.swift:18)
        if (d.slot.init == 1) launch_fill_const_f32((float*)d.slot.dst, d.slot.numel, 1.0f, nullptr);
        if (!d.key.empty()) slots[d.key] = d.slot;
    }
    decls_.clear();
    HIP_CHECK(hipDeviceSynchronize());
    return total + total_w;
}

void ParamTable::view(const std::string& key, void* dst, int kind, long rows, long cols) { slots[key] = make_slot(dst, kind, rows, cols, 0); }

void param_check_shape(const std::string& file_key, const StTensor& t, const ParamSlot& s) {
    const bool shape_ok = t.numel() == s.numel && (!(s.cols && t.shape.size() == 2) || (t.shape[0] == s.rows && t.shape[1] == s.cols));
    if (!shape_ok)
        LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: %s has %ld elements, expected [%ld, %ld]", file_key.c_str(), t.numel(), s.rows,
                  s.cols);
}

void param_upload(const SafeTensors& st, const StTensor& t, const ParamSlot& s, std::vector<uint8_t>* staging) {
    staging->resize(slot_bytes(s));
    if (s.kind == SLOT_BF16) {
        st_to_bf16(st, t, (bf16_t*)staging->data());
    } else {
        float* f = (float*)staging->data();
        st_to_f32(st, t, f);
        for (long i = 0; i < s.numel; ++i) f[i] = host_bf16_to_f32(host_f32_to_bf16(f[i]));
    }
    HIP_CHECK(hipMemcpy(s.dst, staging->data(), staging->size(), hipMemcpyHostToDevice));
}

std::string param_table_load(ltx_ctx* ctx, ParamTable& table, const SafeTensors& st,
                             const std::function<bool(const std::string&, std::string*)>& map_key, bool continue_report) {
    if (!continue_report) ctx->n_loaded = ctx->n_missing = ctx->n_unmatched = 0;
    for (auto& kv : table.slots) kv.second.loaded = false;
    std::vector<uint8_t> staging;
    for (auto& kv : st.tensors) {
        std::string mk;
        if (!map_key(kv.first, &mk)) continue;
        auto it = table.slots.find(mk);
        if (it == table.slots.end()) {
            ctx->n_unmatched++;  // silently dropped by the reference (ModelDownloader.swift:992-1003)
            continue;
        }
        ParamSlot& s = it->second;
        param_check_shape(kv.first, kv.second, s);
        param_upload(st, kv.second, s, &staging);
        if (!s.loaded) ctx->n_loaded++;
        s.loaded = true;
    }
    std::string first_missing;
    for (auto& kv : table.slots)
        if (!kv.second.loaded) {
            if (first_missing.empty()) first_missing = kv.first;
            ctx->n_missing++;
        }
    return first_missing;
}

std::pair<float, float> param_fill_rule_default(const std::string& key, const ParamSlot& slot) {
    const bool is_bias = key.size() > 5 && key.compare(key.size() - 5, 5, ".bias") == 0;
    const bool is_norm = key.find("_norm.weight") != std::string::npos;
    if (slot.kind == SLOT_F32 && is_norm) return {1.0f, 0.02f};
    return {0.f, slot.kind == SLOT_F32 && is_bias ? 0.01f : 0.02f};
}

void param_table_fill_synthetic(ltx_ctx* ctx, ParamTable& table, uint64_t seed, uint64_t first_counter, const ParamFillRule& rule) {
    uint64_t k = first_counter;
    for (auto& kv : table.slots) {
        ParamSlot& s = kv.second;
        const uint64_t sd = seed * 0x9E3779B97F4A7C15ull + (++k) * 0xD1B54A32D192ED03ull;
        const std::pair<float, float> ms = rule(kv.first, s);
        if (s.kind == SLOT_BF16)
            launch_fill_normal_bf16((bf16_t*)s.dst, s.numel, sd, ms.first, ms.second, ctx->stream);
        else
            launch_fill_normal_f32((float*)s.dst, s.numel, sd, ms.first, ms.second, 1, ctx->stream);
        s.loaded = true;
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

void param_export(ltx_ctx* ctx, const ParamSlot& s, float* out) {
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (s.kind == SLOT_F32) {
        HIP_CHECK(hipMemcpy(out, s.dst, (size_t)s.numel * 4, hipMemcpyDeviceToHost));
        return;
    }
    std::vector<bf16_t> h((size_t)s.numel);
    HIP_CHECK(hipMemcpy(h.data(), s.dst, (size_t)s.numel * 2, hipMemcpyDeviceToHost));
    for (long i = 0; i < s.numel; ++i) out[i] = host_bf16_to_f32(h[i]);
}
