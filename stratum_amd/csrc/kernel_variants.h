// kernel_variants.h — the instantiations of the big kernel templates (kernels.h) that exist, as X-macro lists, and the rule
// that picks k_shade's. No HIP in here: kernel_instances.h turns the lists into `extern template` declarations / definitions,
// api.hip into its lookup tables (a variant that is not listed is an error there, never a silent instantiation), and
// tests/cpp/kernel_variants_check.cpp checks the rule against the lists on the host.
#pragma once
#include <stdint.h>

// X(TEXTURED, EXT, LT, MEDIA, PROBE, DEBUG); one list per translation unit (shade_*.hip)
#define STHIP_SHADE_PLAIN(X) \
  X(false, false, false, 0, false, false) X(true, false, false, 0, false, false) X(false, true, false, 0, false, false) X(true, true, false, 0, false, false) \
  X(false, true, false, 0, true, false) X(true, true, false, 0, true, false) X(true, true, false, 0, false, true)
#define STHIP_SHADE_LT(X) \
  X(false, true, true, 0, false, false) X(true, true, true, 0, false, false) X(false, true, true, 0, true, false) X(true, true, true, 0, true, false) X(true, true, true, 0, false, true)
#define STHIP_SHADE_MEDIA(X) \
  X(false, true, false, 1, false, false) X(true, true, false, 1, false, false) X(true, true, false, 1, false, true) X(false, true, false, 2, false, false) X(true, true, false, 2, false, false) \
  X(true, true, false, 2, false, true)
#define STHIP_SHADE_MEDIA_LT(X) X(false, true, true, 1, false, false) X(true, true, true, 1, false, false) X(true, true, true, 1, false, true)
#define STHIP_SHADE_MEDIA_LT2(X) X(false, true, true, 2, false, false) X(true, true, true, 2, false, false) X(true, true, true, 2, false, true)
#define STHIP_SHADE_ALL(X) STHIP_SHADE_PLAIN(X) STHIP_SHADE_LT(X) STHIP_SHADE_MEDIA(X) STHIP_SHADE_MEDIA_LT(X) STHIP_SHADE_MEDIA_LT2(X)
// Y(COUNT, ALPHA, BOUNDED, TOP, WIDE)
#define STHIP_TRACE_ROWS(Y, TOP, WIDE) \
  Y(false, false, false, TOP, WIDE) Y(true, false, false, TOP, WIDE) Y(false, true, false, TOP, WIDE) Y(true, true, false, TOP, WIDE) Y(false, false, true, TOP, WIDE) Y(true, false, true, TOP, WIDE) \
  Y(false, true, true, TOP, WIDE) Y(true, true, true, TOP, WIDE)
// (WIDE = 3, the 4-wide walk over leaf records, exists without ALPHA only: the mask lookup reads per-triangle uvs)
#define STHIP_TRACE_PAIR_ROWS(Y) Y(false, false, false, false, 3) Y(true, false, false, false, 3) Y(false, false, true, false, 3) Y(true, false, true, false, 3)
#define STHIP_TRACE_ALL(Y) STHIP_TRACE_ROWS(Y, false, 0) STHIP_TRACE_ROWS(Y, true, 0) STHIP_TRACE_ROWS(Y, false, 1) STHIP_TRACE_ROWS(Y, false, 2) STHIP_TRACE_PAIR_ROWS(Y)
// Z(TEXTURED, EXT, MEDIA)
#define STHIP_SHADE_LIGHT(Z) Z(false, true, false) Z(true, true, false) Z(false, true, true) Z(true, true, true)

namespace sthip {

// One k_shade instantiation: the template arguments in the order of the lists
struct ShadeVariant {
  bool textured, ext, lt;
  int media;
  bool probe, debug;
};

// The key of a variant in api.hip's tables: the template arguments as bits
constexpr uint32_t shade_key(bool textured, bool ext, bool lt, int media, bool probe, bool debug) {
  return (textured ? 1u : 0u) | (ext ? 2u : 0u) | (lt ? 4u : 0u) | ((uint32_t)media << 3) | (probe ? 32u : 0u) | (debug ? 64u : 0u);
}
constexpr uint32_t trace_key(bool count, bool alpha, bool bounded, bool top, int wide) {
  return (count ? 1u : 0u) | (alpha ? 2u : 0u) | (bounded ? 4u : 0u) | (top ? 8u : 0u) | ((uint32_t)wide << 4);
}
constexpr uint32_t shade_light_key(bool textured, bool ext, bool media) { return (textured ? 1u : 0u) | (ext ? 2u : 0u) | (media ? 4u : 0u); }

// Which k_shade a round of the view pass runs. `textured`: the scene binds images; `ext`: the scene or the flags need the
// extended statements (spheres, an environment, reservoirs, the shading-normal fix); `bdpt`: the paths carry the quantities of
// light-subpath connections; `media`: 0 = no volumes, 1 = their NEE walks are deferred (k_shadow_media), 2 = walked inline;
// `probe`: the launch is a probe of eCoherentRR / eCoherentSampling (never with media: the render call rejects or switches
// off both); `debug`: a BDPTDebugMode is set. A debug mode runs the general (textured, extended) instantiation; its probes
// are the ordinary ones.
constexpr ShadeVariant select_shade_variant(bool textured, bool ext, bool bdpt, int media, bool probe, bool debug) {
  return ShadeVariant{textured || (debug && !probe), ext || debug || probe || bdpt || media != 0, bdpt, media, probe, debug && !probe};
}

// Dynamic LDS of a k_shade launch: the untextured instantiations stage gMaterialData there
constexpr uint32_t shade_lds_bytes(const ShadeVariant& v, uint32_t lds_material_bytes) { return v.textured ? 0u : lds_material_bytes; }

}  // namespace sthip
