// What the engine's device buffers currently hold, as far as the host has to remember it: thirteen validity flags
// and the window of the dilated column list.  Plain C++ (no HIP, no engine), tested without a GPU
// (tests/test_engine_state.py).  The flags are read through the accessors and change ONLY through the transitions below,
// each named after the event that causes it: a new writer of the weights, the phase or the target picks the event it
// is and cannot forget a flag.
#pragma once

namespace hgs {

class EngineState {
public:
    // ---- queries -------------------------------------------------------------------------------------------------
    // G left behind: the last launch of a fused float32 call is row_kernel MODE 3 -- it writes the phase AND the
    // row-transformed field of the next body -- and the next call (or hgs_nearfield2farfield) skips its own first row
    // launch while nothing that G depends on (phase, amplitude, kernel, the column lists it was stored on) has changed.
    //   -1 = gh does not hold G; 0 = G of every column; 1 = of the active columns; 2 = of the dilated active columns
    int gh_state() const { return gh_state_; }
    // need: the columns the next column launch reads (0 / 1 / 2 as above); keep_g: HGS_KEEP_G.  G of every column serves
    // every need, G of the dilated columns serves the active ones while the dilation is the current one
    bool gh_holds(int need, bool keep_g) const {
        return keep_g && (gh_state_ == need || gh_state_ == 0 || (gh_state_ == 2 && need == 1 && dil_valid_));
    }
    bool farfield_valid() const { return farfield_valid_; }   // ff / amp_ff hold the transform of the current nearfield
    bool have_pff() const { return have_pff_; }               // a farfield phase is stored
    bool have_prev() const { return have_prev_; }             // phase_prev holds the phase a one-body fused call started from
    bool w_pending() const { return w_pending_; }             // weights stored un-normalised, wscale holds 1/||w||
    // ... and wscale^2 * sum w^2 = 1 to rounding: the stored weights were last written by an update pass of the fused loop
    // and wscale was folded from THAT pass' partial sums (no NaN left among them).  What the single-inverse MRAF pass
    // builds on (||w'||^2 = 1 + D).  Set by fused_update_done() alone; every other writer of the weights or of wscale is
    // one of the events below that clear it.
    bool w_unit() const { return w_unit_; }
    // spot_update (the N-vector rule) or a folded scale has written weights since the last column scan: a spot whose target
    // and weight were zero then sits in a column the scan found empty, and a NaN factor turns its weight into 1e-4.  The
    // column lists keep their meaning (such a pixel never had a target), the per-column load flags of col_tile2_kernel are
    // withheld until the next scan, which the next dense call that could use them runs itself.
    bool w_outside_scan() const { return w_outside_scan_; }
    bool sparse_dirty() const { return sparse_dirty_; }       // weights or target changed since the last column scan
    bool dil_valid() const { return dil_valid_; }             // the dilated list matches the scan, for the window [dil_lo, dil_hi]
    bool dilation_is(int lo, int hi) const { return dil_valid_ && lo == dil_lo_ && hi == dil_hi_; }
    int dil_lo() const { return dil_lo_; }
    int dil_hi() const { return dil_hi_; }
    bool noise_valid() const { return noise_valid_; }         // the list of NaN-target columns matches the scan
    bool signal_valid() const { return signal_valid_; }       // ... of the columns with a finite non-zero target
    bool ffb_zeroed() const { return ffb_zeroed_; }           // ffb reads as zero outside the NaN-target pixels of that list
    bool cg_have_grad() const { return cg_have_grad_; }       // cg_grad holds the gradient of the last hgs_cg_iterate body

    // ---- uploads -------------------------------------------------------------------------------------------------
    // phase, amplitude, amplitude scalar or propagation kernel: G is dropped as soon as the upload is asked for (before
    // its arguments are looked at), the farfield once the new values are in place
    void nearfield_upload_begins() { gh_state_ = -1; }
    void nearfield_input_changed() { gh_state_ = -1; farfield_valid_ = false; }     // ... and hgs_copy_phase
    void geometry_changed() { farfield_valid_ = false; }                            // compressed: grids, monomials, coefficients
    void target_written() { sparse_dirty_ = true; }                                 // (says nothing about the weights' norm)
    // weights from outside the fused loop (host / device upload, sparse upload, hgs_reset_weights): a dense upload dirties
    // the scan from the moment it is issued (a failed one may have written part of the array) ...
    void weights_write_begins() { sparse_dirty_ = true; }
    // ... and once they are in place and wscale is back to 1, they are whatever the caller gave
    void weights_written() { sparse_dirty_ = true; w_pending_ = false; w_unit_ = false; }
    // normalize_weights_now: wscale multiplied into the stored weights, then reset to 1 (a non-finite scale -- all weights
    // zero -- turns the zeros of every column into NaN, hence "outside the scan")
    void scale_folded() { w_outside_scan_ = true; w_pending_ = false; w_unit_ = false; }
    void phase_ff_stored() { have_pff_ = true; }                                    // uploaded, or stored by a pass

    // ---- transforms and the general operators ----------------------------------------------------------------------
    void farfield_materialised(bool stored_pff) { if (stored_pff) have_pff_ = true; farfield_valid_ = true; }
    void farfield_consumed() { farfield_valid_ = false; }          // the inverse ran: ff holds the constrained field, the phase moved on
    void general_rule_updated_weights() { sparse_dirty_ = true; }  // the general rules rewrite the weight array
    void cg_gradient_stored() { cg_have_grad_ = true; }

    // ---- the fused loops -------------------------------------------------------------------------------------------
    void fused_call_begins() { farfield_valid_ = false; }
    // spot_update writes the weights itself, at pixels the scan may have found empty
    void spot_sparse_call_begins() { farfield_valid_ = false; w_unit_ = false; w_outside_scan_ = true; }
    // a dense call that could use the per-column load flags scans again, once, after weights written behind the scan's back
    void rescan_if_written_outside() { if (w_outside_scan_) sparse_dirty_ = true; }
    void column_pass_begins() { gh_state_ = -1; }                  // it turns G into H in place
    // the update pass of the fused loop wrote the weights; wscale comes from this pass' partials, in the pass or in the row
    // launch that closes the body.  The only way to w_unit
    void fused_update_done() { w_pending_ = true; w_unit_ = true; }
    void row_launch_begins() { gh_state_ = -1; }
    // mode: row_kernel MODE (1 extracts the phase and leaves no G); store_sparse: the columns it stored, as gh_state counts them
    void row_stored_g(int mode, int store_sparse) { if (mode != 1) gh_state_ = store_sparse; }
    void prev_phase_kept() { have_prev_ = true; }
    // a call of several bodies, the general loop, hgs_cg_iterate, the option switched off: nothing describes "the phase before"
    void prev_phase_dropped() { have_prev_ = false; }

    // ---- column scan and the lists derived from it -------------------------------------------------------------------
    void scan_started() { if (gh_state_ > 0) gh_state_ = -1; }     // (a G stored on the old column lists; one of every column stays good)
    void scan_finished() {      // the lists derived from the old scan go with it
        sparse_dirty_ = w_outside_scan_ = false;
        dil_valid_ = noise_valid_ = signal_valid_ = false;
    }
    void dilation_rebuild_begins() { if (gh_state_ == 2) gh_state_ = -1; }
    void dilation_rebuilt(int lo, int hi) { dil_lo_ = lo; dil_hi_ = hi; dil_valid_ = true; }
    void signal_list_rebuilt() { signal_valid_ = true; }
    // the noise columns moved: ffb must read as zero outside THEIR NaN-target pixels, so it is zeroed again before use
    void noise_list_rebuild_begins() { ffb_zeroed_ = false; }
    void noise_list_rebuilt() { noise_valid_ = true; }
    void ffb_was_zeroed() { ffb_zeroed_ = true; }

    // ---- hgs_reset, hgs_set_option -------------------------------------------------------------------------------------
    // Hologram.reset: phase_ff / farfield / amp_ff back to "None"; a kept G is the un-extracted phasor of the last body and a
    // reset hologram starts from its phase, like a new one; no gradient is held (the weights follow: weights_written)
    void reset_state() {
        have_pff_ = have_prev_ = farfield_valid_ = cg_have_grad_ = false;
        gh_state_ = -1;
    }
    // hgs_set_option says which kind of option it changed: one that may change which columns the next launch expects in gh,
    // one that changes what the column scan rounds to
    void column_policy_changed() { gh_state_ = -1; }
    void scan_policy_changed() { sparse_dirty_ = true; }

private:
    int gh_state_ = -1;
    bool farfield_valid_ = false, have_pff_ = false, have_prev_ = false;
    bool w_pending_ = false, w_unit_ = false, w_outside_scan_ = false;
    bool sparse_dirty_ = true, dil_valid_ = false, noise_valid_ = false, signal_valid_ = false, ffb_zeroed_ = false;
    bool cg_have_grad_ = false;
    int dil_lo_ = 0, dil_hi_ = 0;
};

}  // namespace hgs
