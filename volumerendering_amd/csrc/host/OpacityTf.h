// OpacityTF -- 1-D opacity transfer function (R32Float[R]).  Mirrors med::OpacityTF
// (App/src/tf/OpacityTf.h:14-67, OpacityTf.cpp) minus the ImPlot editor.
#pragma once
#include <array>
#include <memory>

#include "TransferFunction.h"
#include "VolumeFile.h"

namespace med {

class OpacityTF : public TransferFunction {
public:
    explicit OpacityTF(int desiredTfResolution);  // 0 = maximal resolution

    void UpdateTexture() override;
    void ActivateHistogram(const VolumeFile& file);  // OpacityTf.cpp:144-179
    // The same from the device histogram of volume `slot` of ctx (vr_histogram: channel 3, the whole volume, CLAMP), for volumes that
    // were prepared on the device; `normalized` and `dataRange` are what file.IsNormalized() / file.GetDataRange() say of a host volume.
    // The CPU overload counts in float, whose ++ saturates at 2^24; this one converts each exact u64 count to float with one correct
    // rounding and does not saturate.  The two agree bit for bit whenever every bin is below 2^24.  Returns a vr_status.
    int ActivateHistogram(vr_ctx* ctx, int slot, bool normalized, size_t dataRange);
    std::string GetType() const override { return "opacity"; }
    bool Save(const std::string& name) override;     // :181-198
    void Load(const std::string& name, TFLoadOption option = TFLoadOption::NONE) override;  // :200-314
    void ResetTF() override;                          // :29-45
    void CalibrateOnMask(std::shared_ptr<const VolumeFile> mask, std::shared_ptr<const VolumeFile> file,
                         std::array<int, 4> activeContours);  // :316-487
    // The same from the device histogram of `channel` of volume fileSlot inside the contours of volume maskSlot (vr_histogram: DROP,
    // scale 1, bins = maxValue <= VR_HIST_MAX_BINS; the active contours' rows are summed, keeping multiplicity).  channel 3 is the CPU
    // overload's .a and must run before normalisation; channel 0 calibrates after vr_volume_normalize, because the raw value
    // survives in .r.  Returns a vr_status; the table stays as it was where the CPU overload returns early.
    int CalibrateOnMask(vr_ctx* ctx, int fileSlot, int maskSlot, int channel, size_t maxValue, std::array<int, 4> activeContours);

    // editor surface without ImPlot: what a click / drag on the plot does
    void SetControlPoint(int cpId, double x, double y);  // DragPoint + CheckDragBounds + UpdateYAxis (:74-94)

    const std::vector<float>& GetYPoints() const { return m_YPoints; }
    const std::vector<float>& GetHistogram() const { return m_Histogram; }

private:
    void UpdateYAxis(int cpId) override;  // :489-523
    void CalibrateFromBins(const std::vector<double>& bin, size_t maxNumber);  // the control-point half of CalibrateOnMask

    std::vector<float> m_XPoints{};
    std::vector<float> m_YPoints{};
    std::vector<float> m_Histogram{};
};

}  // namespace med
