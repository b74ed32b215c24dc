// cf_decays_mc.h -- what the sampler's batch loop (cf_sampler.hip) needs of the Monte Carlo decays (cf_decays_mc.hip): the one-pass
// decay-and-bin launch on a device-resident table (is3d_decay_mc_table), and the checks both of its entries make before any device use.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/is3d_amd.h"
#include "cf_sampler_bins.h"
#include "cf_sampler_flow.h"
#include "cf_sampler_flow_diff.h"
#include "cf_sampler_pairs.h"
#include "cf_sampler_hbt.h"

namespace is3d {

// the run-wide words of cf_decay_mc_bins: decays, stuck, trials, exhausted, stack overflows (never), final particles
constexpr int kDecayMcBinTallies = 6;

// A decayed-and-binned run on the device: the table, the slot map (DEVICE, one int32 per table entry, -1 = not binned), the bins with what
// follows from them for n_slots species, and the device block  hist [layout.total] | yield [n_events] | tally [kDecayMcBinTallies].
struct DecayMcBinRun {
    const is3d_decay_mc_table *table;
    const int32_t *slot_dev;
    int32_t n_slots, n_events;
    uint64_t seed;
    int32_t lifetime;
    is3d_sampler_test_bins bins;
    SamplerBinWidths widths;
    SamplerHistLayout layout;
    unsigned long long *block_dev;
};

// the private form keeps its tally words in static LDS beside the dynamic block: it fits when block + kDecayMcBinTallies words <= 64 KiB
inline bool decay_mc_bins_lds_fits(const SamplerHistLayout &l) { return l.total + kDecayMcBinTallies <= (int64_t)(65536 / sizeof(unsigned long long)); }

// IS3D_EINVAL, no device use: n_slots < 1, a NULL map, a slot outside [-1, n_slots), bins->kernel_form = 2 on a block of n_slots species
// that does not fit (bins and hist themselves: sampler_check_bin_args)
int decay_mc_check_slots(int32_t n_entries, const int32_t *slot, int32_t n_slots, const is3d_sampler_test_bins *bins);
// every refusal of is3d_decay_mc_table_create, and nothing else: the host analysis of a table without a device
int decay_mc_table_check(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id);
int32_t decay_mc_table_entries(const is3d_decay_mc_table *t);
int32_t decay_mc_table_chosen(const is3d_decay_mc_table *t);
int decay_mc_table_device(const is3d_decay_mc_table *t);
// n primaries of a DEVICE list (species indexing the table's chosen list, ordered by event), primary i drawing from stream first_particle + i,
// decayed and binned into r.block_dev on the null stream in the form r.bins.kernel_form (0 = private where it fits, 1 = global, 2 = private)
hipError_t decay_mc_bins_launch(const DecayMcBinRun &r, const is3d_particle *primaries_dev, int64_t n, int64_t first_particle);
// A decayed run into flow records (cf_sampler_flow.h): the slot map as above, the cuts with their thresholds, and the device block
// records [n_events * n_slots * 51] | tally [kDecayMcBinTallies].  The private form keeps its window beside the static tally words.
struct DecayMcFlowRun {
    const is3d_decay_mc_table *table;
    const int32_t *slot_dev;
    int32_t n_slots, n_events;
    uint64_t seed;
    int32_t lifetime;
    is3d_flow_cuts cuts;
    FlowThresholds thresholds;
    unsigned long long *block_dev;
    // differential records (cf_sampler_flow_diff.h) instead: n_pT > 0 bins on the DEVICE edge table edges_dev[n_pT + 1]; the block then holds
    // n_events * n_slots * n_pT * 51 words and the window stands beside the staged edges as well
    int32_t n_pT = 0;
    const double *edges_dev = nullptr;
};
// as decay_mc_bins_launch, every final particle going to the rule of cf_sampler_flow.h; form r.cuts.kernel_form
hipError_t decay_mc_flow_launch(const DecayMcFlowRun &r, const is3d_particle *primaries_dev, int64_t n, int64_t first_particle);
// A decayed run into pair occupancies (cf_sampler_pairs.h): the slot map as above, the bins with their tables, and the device block
// tally [kDecayMcBinTallies 64-bit words] | occ [n_events * n_slots * n_y * n_phi 32-bit words]
struct DecayMcPairRun {
    const is3d_decay_mc_table *table;
    const int32_t *slot_dev;
    int32_t n_slots, n_events;
    uint64_t seed;
    int32_t lifetime;
    is3d_pair_bins bins;
    PairTables tables;
    unsigned long long *tally_dev;
    unsigned *occ_dev;
};
// as decay_mc_bins_launch, every final particle going to the rule of cf_sampler_pairs.h and making ONE occupancy add
hipError_t decay_mc_pairs_launch(const DecayMcPairRun &r, const is3d_particle *primaries_dev, int64_t n, int64_t first_particle);
// A decayed run into HBT records (cf_sampler_hbt.h): the slot map as above; every final particle goes to the single-particle rule and an
// accepted one to hbt_select_put of `run` -- the count pass (fill = false, which also adds the tallies to tally_dev
// [kDecayMcBinTallies 64-bit words]) or the fill pass over the same counter-based stream, which sees the same finals
struct DecayMcHbtRun {
    const is3d_decay_mc_table *table;
    const int32_t *slot_dev;
    uint64_t seed;
    int32_t lifetime;
    unsigned long long *tally_dev;
};
hipError_t decay_mc_hbt_launch(const DecayMcHbtRun &r, const HbtRun &run, const is3d_particle *primaries_dev, int64_t n, int64_t first_particle,
                               bool fill);
// a whole batch: batch_begin, the count pass, batch_plan, the fill pass, batch_pairs
int decay_mc_hbt_batch(const DecayMcHbtRun &r, HbtRun &run, const is3d_particle *primaries_dev, int64_t n, int64_t first_particle);
// the tallies of a finished run (HOST copy of the tally words) into stats; IS3D_EINVAL if a pending stack overflowed
int decay_mc_bins_tallies(const unsigned long long *tally, is3d_decay_mc_stats *stats);
// the static part of the stats: what the table analysis found
void decay_mc_table_stats(const is3d_decay_mc_table *t, is3d_decay_mc_stats *stats);

}  // namespace is3d
