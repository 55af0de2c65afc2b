"""D-NeRF backbone (dnerf/ of the reference): a deformation field over time in front of the NGP density and colour heads."""
