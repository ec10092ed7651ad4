"""The part of the reference's inpaint/ package that is per-pixel work: bilateral_filtering, the depth preparation in front of the
mesh code.  The mesh stages and the inpainting networks are not here."""
