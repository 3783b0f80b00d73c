// kernel_variants_check.cpp — the rule that picks k_shade's instantiation (csrc/kernel_variants.h: select_shade_variant) against
// the lists of instantiations that are compiled, and against the if/else ladders the rule replaced. Host only.
//   a) every variant the rule selects for a reachable input is in the STHIP_SHADE_* lists
//   b) every listed variant is selected by some reachable input
//   c) the rule and its LDS size agree with `ladder` below, the ladders written out case by case
// Reachable: textured x ext x bdpt x media {0, 1, 2} x probe x debug, without probe && media (eCoherentRR is off with media,
// eCoherentSampling with media is rejected).
#include <stdio.h>

#include <set>

#include "../../stratum_amd/csrc/kernel_variants.h"

using sthip::shade_key;

struct Launch {
  uint32_t key, lds;
};

// The ladders as they stood in the render call before the rule: the probe's (by bdpt, then textured) and the round's (debug;
// media && bdpt; media inline; media; bdpt; textured && ext; textured; ext; plain). `lds` is what the launch passed as dynamic LDS.
static Launch ladder(bool textured, bool ext, bool bdpt, int media, bool probe, bool debug, uint32_t shade_lds) {
  const bool inline_media = media == 2;
  if (probe) {
    if (bdpt) {
      if (textured) return {shade_key(true, true, true, 0, true, false), 0};
      return {shade_key(false, true, true, 0, true, false), shade_lds};
    }
    if (textured) return {shade_key(true, true, false, 0, true, false), 0};
    return {shade_key(false, true, false, 0, true, false), shade_lds};
  }
  if (debug) {
    if (media && bdpt && inline_media) return {shade_key(true, true, true, 2, false, true), 0};
    if (media && bdpt) return {shade_key(true, true, true, 1, false, true), 0};
    if (media && inline_media) return {shade_key(true, true, false, 2, false, true), 0};
    if (media) return {shade_key(true, true, false, 1, false, true), 0};
    if (bdpt) return {shade_key(true, true, true, 0, false, true), 0};
    return {shade_key(true, true, false, 0, false, true), 0};
  }
  if (media && bdpt) {
    if (textured && inline_media) return {shade_key(true, true, true, 2, false, false), 0};
    if (textured) return {shade_key(true, true, true, 1, false, false), 0};
    if (inline_media) return {shade_key(false, true, true, 2, false, false), shade_lds};
    return {shade_key(false, true, true, 1, false, false), shade_lds};
  }
  if (media && inline_media) {
    if (textured) return {shade_key(true, true, false, 2, false, false), 0};
    return {shade_key(false, true, false, 2, false, false), shade_lds};
  }
  if (media) {
    if (textured) return {shade_key(true, true, false, 1, false, false), 0};
    return {shade_key(false, true, false, 1, false, false), shade_lds};
  }
  if (bdpt) {
    if (textured) return {shade_key(true, true, true, 0, false, false), 0};
    return {shade_key(false, true, true, 0, false, false), shade_lds};
  }
  if (textured && ext) return {shade_key(true, true, false, 0, false, false), 0};
  if (textured) return {shade_key(true, false, false, 0, false, false), 0};
  if (ext) return {shade_key(false, true, false, 0, false, false), shade_lds};
  return {shade_key(false, false, false, 0, false, false), shade_lds};
}

int main() {
  std::set<uint32_t> listed, selected;
  size_t entries = 0;
#define ADD(T, E, L, M, P, D) listed.insert(shade_key(T, E, L, M, P, D)), entries++;
  STHIP_SHADE_PLAIN(ADD) STHIP_SHADE_LT(ADD) STHIP_SHADE_MEDIA(ADD) STHIP_SHADE_MEDIA_LT(ADD) STHIP_SHADE_MEDIA_LT2(ADD)
#undef ADD
  int bad = 0;
  if (listed.size() != entries) bad++, printf("the lists name %zu variants, %zu of them distinct\n", entries, listed.size());
  const uint32_t material_bytes = 4096;  // what an untextured scene stages in LDS (0 for a textured one, as the render call computes it)
  for (int bits = 0; bits < 32; bits++)
    for (int media = 0; media < 3; media++) {
      const bool textured = bits & 1, ext = bits & 2, bdpt = bits & 4, probe = bits & 8, debug = bits & 16;
      if (probe && media) continue;
      const uint32_t shade_lds = textured ? 0u : material_bytes;
      const sthip::ShadeVariant v = sthip::select_shade_variant(textured, ext, bdpt, media, probe, debug);
      const uint32_t key = shade_key(v.textured, v.ext, v.lt, v.media, v.probe, v.debug);
      selected.insert(key);
      if (!listed.count(key)) bad++, printf("(a) not listed: k_shade<%d, %d, %d, %d, %d, %d>\n", v.textured, v.ext, v.lt, v.media, v.probe, v.debug);
      const Launch was = ladder(textured, ext, bdpt, media, probe, debug, shade_lds);
      if (was.key != key || was.lds != sthip::shade_lds_bytes(v, shade_lds))
        bad++, printf("(c) textured %d ext %d bdpt %d media %d probe %d debug %d: the ladder ran key %u with %u B of LDS, the rule says key %u with %u B\n", textured, ext, bdpt, media, probe, debug, was.key, was.lds, key,
                      sthip::shade_lds_bytes(v, shade_lds));
    }
  for (uint32_t key : listed)
    if (!selected.count(key)) bad++, printf("(b) listed but never selected: key %u\n", key);
  if (bad) return 1;
  printf("VARIANTS OK: %zu listed, %zu selected\n", listed.size(), selected.size());
  return 0;
}
