/*
 * integrator_props.h — the one mapping of the reference integrator's properties to ppg_config: names and defaults verbatim from
 * GuidedPathTracer(const Properties &), GP:1014-1085, and MonteCarloIntegrator (integrator.cpp:190-225).  Used by GuidedPathTracerHIP's
 * constructor (guided_path_hip.h) and by PluginCore::configure (plugin_core.h); `seed`, `dumpPrefix` and `adamRegions` differ between
 * the two and stay with them.
 */
#ifndef PPG_INTEGRATOR_PROPS_H
#define PPG_INTEGRATOR_PROPS_H

#include <string>

#include "../../include/ppg.h"

namespace ppg {

// ppg_config's six enum strings point into storage their owner keeps next to it
inline void pointEnumStrings(ppg_config &cfg, const std::string (&s)[6]) {
    cfg.nee = s[0].c_str(); cfg.sampleCombination = s[1].c_str(); cfg.spatialFilter = s[2].c_str();
    cfg.directionalFilter = s[3].c_str(); cfg.bsdfSamplingFractionLoss = s[4].c_str(); cfg.budgetType = s[5].c_str();
}

// P: anything with Mitsuba's typed getters (mitsuba::Properties; ppg::Properties of guided_path_hip.h)
template <class P> void readIntegratorProperties(const P &props, ppg_config &cfg, std::string (&s)[6]) {
    s[0] = props.getString("nee", "never");
    s[1] = props.getString("sampleCombination", "automatic");
    s[2] = props.getString("spatialFilter", "nearest");
    s[3] = props.getString("directionalFilter", "nearest");
    s[4] = props.getString("bsdfSamplingFractionLoss", "none");
    s[5] = props.getString("budgetType", "seconds");
    pointEnumStrings(cfg, s);
    cfg.sdTreeMaxMemory = props.getInteger("sdTreeMaxMemory", -1);
    cfg.sTreeThreshold = props.getInteger("sTreeThreshold", 12000);
    cfg.dTreeThreshold = props.getFloat("dTreeThreshold", 0.01f);
    cfg.bsdfSamplingFraction = props.getFloat("bsdfSamplingFraction", 0.5f);
    cfg.sppPerPass = props.getInteger("sppPerPass", 4);
    cfg.budget = props.getFloat("budget", 300.0f);
    cfg.dumpSDTree = props.getBoolean("dumpSDTree", false);
    cfg.rrDepth = props.getInteger("rrDepth", 5);  // MonteCarloIntegrator, integrator.cpp:192-218
    cfg.maxDepth = props.getInteger("maxDepth", -1);
    cfg.strictNormals = props.getBoolean("strictNormals", false);
    cfg.hideEmitters = props.getBoolean("hideEmitters", false);
    cfg.device = props.getInteger("device", 0);
}

}  // namespace ppg
#endif
