# tools/test_supernet.py with per-subnet BatchNorm re-calibration: the model-space rules of
# fcn_ar50to101v2_test_supernet.py, each selected subnet scored under running statistics that were
# re-estimated for it.  Before a subnet is evaluated, num_batches batches of
# data.train (training pipeline, seeded, the same batches for every subnet and on every rank) are run
# forward on batch statistics and their cumulative average is written into the slices the subnet
# reads; the supernet's blended statistics are put back bit for bit afterwards.  Run it with
#   python tools/test_supernet.py <this file> CHECKPOINT --model-space-path flops.json \
#          --metric-tag calibrated
# so the columns are metric.calibrated.* next to any metric.direct.* the model-space file carries.
# num_batches=32 is an untuned starting value: no ranking quality has been measured with it.
_base_ = ['./fcn_ar50to101v2_test_supernet.py']
caliberate_bn = dict(recalibrate=dict(num_batches=32, samples_per_gpu=None, seed=0))
