"""The bound on the gradient of the cSSIM loss (tests/test_cssim_loss_host.py on the CPU, tests/test_gpu_cssim_loss.py on the GPU), as a
fraction of the sample's max |gradient|.

CSSIM_GRAD_MODEL: per family of tests/cssim_grad_ref.CASES, the largest error of the float32 numpy MODEL of the kernel's centred algebra
(cssim_grad_ref.grad_f32) against the fp64 restatement (cssim_grad_ref.grad), rounded up to two digits; the CPU test recomputes them.
CSSIM_GRAD_TOL: 4 x the largest of them, rounded up to one significant digit - the margin the project gave CSSIM_TOL_PIN, here for the
kernel's different summation order, its fused multiply-adds and the seeds not listed: 4 x 1.5e-6 = 6.0e-6 -> 6e-6.  It is derived from
the CPU model, never from the kernel's own error.
CSSIM_GRAD_MEASURED: the kernel's own largest error per family on an MI355X, written beside it for the record only."""
CSSIM_GRAD_MODEL = {"shapes": 1.5e-6, "holes": 1.2e-6, "borders": 1.0e-6, "options": 6.6e-7, "conditioning": 4.8e-7}
CSSIM_GRAD_TOL = 6e-6
CSSIM_GRAD_MEASURED = {"shapes": (2.17e-6, "one-pixel-map-gaussian[1]"), "holes": (1.12e-6, "holes-49x71-gaussian[0]"),
                       "borders": (7.54e-7, "border8-gaussian[0]"), "options": (6.13e-7, "no-bias-gaussian[1]"),
                       "conditioning": (5.11e-7, "cond-24x24-gaussian-L0.9-c0.05-blob[0]")}
