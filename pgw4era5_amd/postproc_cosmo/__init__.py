"""COSMO-specific post-processing (the reference's postproc_cosmo/): `extpar_adapt` perturbs the deep soil temperature
climatology T_CL of an extpar file with the annual mean of the ts climate delta."""
