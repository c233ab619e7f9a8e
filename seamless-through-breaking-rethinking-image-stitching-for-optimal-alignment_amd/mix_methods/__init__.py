"""`mix_fn` plug-ins of the TPS post-pipeline (reference: core/inference/mix_methods/<name>.py, selected by
`TPS_PIPELINE_CONFIG.mix_method`, out.py:235): same module names, same `mix_fn` signature and return tuple.  The mask /
image algebra runs in HIP kernels; the inpainter is whatever object the caller passes (`.name`, `.inpaint(...)`, the
reference's protocol: core/inference/mix_methods/utils/transref_inpainter.py:16,37).  `utils.transref_inpainter` is the TransRef
network on the GPU (`stitch_amd.transref`; its module-level `inpainter` needs the reference's `400_Trans.pth`, without it the import
raises ImportError); the diffusion and GAN inpainters are out of scope and `utils.passthrough_inpainter` stands in for them.
`utils.cv_inpainter` is the reference's weight-free OpenCV Telea inpainter on the GPU (`ops.inpaint_telea`)."""
